"""CPU checks of the dense polynomial commitment seam (include/spg.h spg_poly_*): the entry points are declared and
exported, the tests' checker (tests/polyeval_ref.py over the oracle's headers) proves what the oracle's own verifiers
accept, its blinded bound is the plain-integer sum, and the product's grouping plan (csrc/pe_plan.hpp through
spgh_pe_plan) gives the groups, first-seen order and coefficient exponents the oracle's provers derive; the
disjoint-rounds walk (spgh_pe_walk_disjoint) against the reference's rule stated in plain Python."""
import ctypes
import os
import re

import numpy as np
import pytest

import fieldref as fr
import polyeval_cases as pc
import polyeval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg.so")
HOSTCHECK = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg_hostcheck.so")
HDR = os.path.join(ROOT, "include", "spg.h")

POLY_SYMBOLS = ["spg_poly_gens_new", "spg_poly_gens_n", "spg_poly_gens_download", "spg_poly_gens_free",
                "spg_poly_commit", "spg_poly_eval_prove", "spg_poly_eval_verify", "spg_poly_eval_verify_plain",
                "spg_poly_eval_prove_batched_points", "spg_poly_eval_verify_plain_batched_points",
                "spg_poly_eval_prove_batched_instances", "spg_poly_eval_verify_plain_batched_instances"]
LABEL, TLABEL = b"gens_polyeval_test", b"polyeval_test"


@pytest.fixture(scope="module")
def seed(oracle):
    import workload

    return workload.tape_seed()


def test_poly_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(spg_[a-z0-9_]+)\s*\(", src))
    assert not [s for s in POLY_SYMBOLS if s not in declared]
    assert sorted(s for s in declared if s.startswith("spg_poly_")) == sorted(POLY_SYMBOLS)
    lib = ctypes.CDLL(LIB)
    assert not [s for s in POLY_SYMBOLS if not hasattr(lib, s)]


@pytest.mark.parametrize("nv,blinded", [(1, False), (3, True), (4, False), (4, True)])
def test_checker_single_proof_verifies(oracle, seed, nv, blinded):
    Z, r = pc.scalars(100 + nv, 1 << nv), pc.scalars(200 + nv, nv)
    Zr = pc.evaluate(Z, r, nv)
    bl = pc.scalars(300 + nv, 1 << (nv // 2)) if blinded else None
    bz = pc.scalars(400 + nv, 1)[0] if blinded else None
    good = ref.prove(LABEL, nv, TLABEL, seed, Z, r, Zr, bl, bz)
    assert good.verified and len(good.proof) == 2 * (8 + 32 * (nv - nv // 2)) + 128
    bad = ref.prove(LABEL, nv, TLABEL, seed, Z, r, Zr, bl, bz, tamper=True)
    assert bad.proof == good.proof and not bad.verified
    wrong = ref.prove(LABEL, nv, TLABEL, seed, Z, r, pc.scalars(1, 1)[0], bl, bz)
    assert not wrong.verified
    # the blinds enter the proof and the commitment
    if blinded:
        assert good.proof != ref.prove(LABEL, nv, TLABEL, seed, Z, r, Zr).proof
        assert not np.array_equal(ref.commit(LABEL, nv, Z, nv, bl), ref.commit(LABEL, nv, Z, nv))


def test_checker_batched_points_verify(oracle, seed):
    nv = 4
    Z, rl = pc.scalars(110, 1 << nv), pc.points(5, nv, pc.ABACBA)
    Zr = np.array([pc.evaluate(Z, r, nv) for r in rl])
    good = ref.prove_points(LABEL, nv, TLABEL, seed, Z, nv, rl, Zr)
    assert good.verified and good.nproofs == 3
    assert not ref.prove_points(LABEL, nv, TLABEL, seed, Z, nv, rl, Zr, tamper=True).verified
    Zr[2] = pc.scalars(2, 1)[0]
    assert not ref.prove_points(LABEL, nv, TLABEL, seed, Z, nv, rl, Zr).verified


@pytest.mark.parametrize("name", ["padtrim", "forty"])
def test_checker_batched_instances_verify(oracle, seed, name):
    nvs, rl = pc.instance_cases()[name]
    Zs = pc.instance_polys(700, nvs)
    Zr = np.array([pc.evaluate(Z, r, nv) for Z, r, nv in zip(Zs, rl, nvs)])
    good = ref.prove_instances(LABEL, max(nvs), TLABEL, seed, Zs, nvs, rl, Zr)
    assert good.verified and good.nproofs == {"padtrim": 1, "forty": 5}[name]
    assert not ref.prove_instances(LABEL, max(nvs), TLABEL, seed, Zs, nvs, rl, Zr, tamper=True).verified


@pytest.mark.parametrize("nv", [1, 3, 4, 7])
def test_checker_blinded_bound_is_the_integer_sum(oracle, nv):
    """LZ[c] = sum_j L[j] Z[j Rs + c] and LZ_blind = sum_j blinds[j] L[j] over plain integers mod q, L the eq table of
    the point's left half (index bit of r[0] most significant)"""
    ln = nv // 2
    Ls, Rs = 1 << ln, 1 << (nv - ln)
    Zm, rm, bm = pc.scalars(120 + nv, 1 << nv), pc.scalars(220 + nv, nv), pc.scalars(320 + nv, Ls)
    Z, r, b = ([fr.from_mont(x) for x in fr.ints(a)] for a in (Zm, rm, bm))
    L = [1]
    for rj in r[:ln]:
        L = [v for e in L for v in (e * (1 - rj) % fr.Q, e * rj % fr.Q)]
    LZ = [sum(L[j] * Z[j * Rs + c] for j in range(Ls)) % fr.Q for c in range(Rs)]
    got, got_b = ref.bound(Zm, rm, bm)
    assert [fr.from_mont(x) for x in fr.ints(got)] == LZ
    assert fr.from_mont(fr.ints(got_b)[0]) == sum(x * y for x, y in zip(b, L)) % fr.Q
    assert fr.ints(ref.bound(Zm, rm)[1]) == [0]


# ---------------------------------------------------------------- the product's plan
def plan(nv_list, r_list, instances):
    hc = ctypes.CDLL(HOSTCHECK)
    hc.spgh_pe_plan.restype = ctypes.c_long
    n = len(r_list)
    nvs = list(nv_list) if instances else [nv_list[0]] * n
    term = (ctypes.c_size_t * (6 * n))()
    grp = (ctypes.c_size_t * (7 * n))()
    tot = (ctypes.c_size_t * 4)()
    fitted = np.zeros((sum(nvs), 4), np.uint64)
    rl = np.ascontiguousarray(np.concatenate([np.asarray(r, np.uint64).reshape(-1, 4) for r in r_list]))
    lens = (ctypes.c_size_t * n)(*[len(r) for r in r_list])
    k = hc.spgh_pe_plan(ctypes.c_int(1 if instances else 0), ctypes.c_size_t(n),
                        (ctypes.c_size_t * len(nv_list))(*nv_list), rl.ctypes.data_as(ctypes.c_void_p), lens, term,
                        fitted.ctypes.data_as(ctypes.c_void_p), grp, tot)
    terms = [tuple(term[6 * i:6 * i + 6]) for i in range(n)]
    groups = [tuple(grp[7 * g:7 * g + 7]) for g in range(k)]
    return terms, groups, fitted, tuple(tot)


def check_plan(nv_list, r_list, instances):
    g, e, fitted, k = ref.groups(nv_list, r_list, instances)
    terms, groups, pfit, (part_len, out_len, xblocks, nbytes) = plan(nv_list, r_list, instances)
    assert len(groups) == k
    assert [t[0] for t in terms] == g and [t[1] for t in terms] == e
    assert np.array_equal(pfit, fitted)
    # groups in first-seen order, each opened by its first term, with the reference's shapes
    nvs = list(nv_list) if instances else [nv_list[0]] * len(r_list)
    for gi, (nv, Ls, Rs, first, S, part_off, out_off) in enumerate(groups):
        assert first == g.index(gi) and nv == nvs[first] and Ls == 1 << (nv // 2) and Rs == 1 << (nv - nv // 2)
    # slabs: every bound term covers its Ls rows exactly, a group's slabs are contiguous, groups follow one another
    po = oo = 0
    for gi, (nv, Ls, Rs, first, S, part_off, out_off) in enumerate(groups):
        assert (part_off, out_off) == (po, oo)
        slab = 0
        for t in [t for t in terms if t[0] == gi and t[2]]:
            assert t[5] == slab and t[3] >= 1 and (t[3] - 1) * t[4] < Ls <= t[3] * t[4]
            slab += t[3]
        assert slab == S
        po, oo = po + S * Rs, oo + Rs
    assert (part_len, out_len) == (po, oo)
    # bound terms: all of them in the instances form, the group openers in the points form
    assert [bool(t[2]) for t in terms] == [instances or x == 0 for x in e]
    assert nbytes == 8 + sum(2 * (8 + 32 * (Rs.bit_length() - 1)) + 128 for (_, _, Rs, *_) in groups)
    return terms, groups


def test_plan_points_abacba(oracle):
    terms, groups = check_plan([11], pc.points(7, 11, pc.ABACBA), False)
    assert [t[0] for t in terms] == pc.ABACBA_GROUPS and [t[1] for t in terms] == pc.ABACBA_EXPS
    assert len(groups) == 3
    # one point, and more distinct left halves than one pass feeds
    assert len(check_plan([4], pc.points(8, 4, "a"), False)[1]) == 1
    terms, groups = check_plan([11], pc.points(9, 11, "abcdea"), False)
    assert len(groups) == 5 and [t[1] for t in terms] == [0, 0, 0, 0, 0, 1]


def walk_disjoint(shapes):
    hc = ctypes.CDLL(HOSTCHECK)
    hc.spgh_pe_walk_disjoint.restype = ctypes.c_long
    n = len(shapes)
    group, exp = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    flat = (ctypes.c_size_t * (2 * n))(*[x for s in shapes for x in s])
    k = hc.spgh_pe_walk_disjoint(ctypes.c_size_t(n), flat, group, exp)
    return list(group), list(exp), k


def disjoint_rule(shapes):
    """prove_batched_instances_disjoint_rounds (dense_mlpoly.rs:861-960) in plain Python: a map from (num_proofs,
    num_inputs) to a slot; a repeat first advances the one running exponent, then joins its slot with it"""
    slots, group, exp, e = {}, [], [], 0
    for key in shapes:
        if key in slots:
            e += 1
            exp.append(e)
        else:
            slots[key] = len(slots)
            exp.append(0)
        group.append(slots[key])
    return group, exp, len(slots)


A, B, C = (4, 8), (2, 8), (4, 4)
DISJOINT_CASES = {
    "one": ([A], [0], [0]),
    "one_key": ([A, A, A], [0, 0, 0], [0, 1, 2]),
    "distinct": ([A, B, C, (8, 8)], [0, 1, 2, 3], [0, 0, 0, 0]),
    "abacba": ([A, B, A, C, B, A], [0, 1, 0, 2, 1, 0], [0, 0, 1, 0, 2, 3]),
    "num_inputs_differs": ([(4, 8), (4, 16)], [0, 1], [0, 0]),
    "num_proofs_differs": ([(4, 8), (8, 8)], [0, 1], [0, 0]),
}


@pytest.mark.parametrize("name", list(DISJOINT_CASES))
def test_walk_disjoint(name):
    shapes, groups, exps = DISJOINT_CASES[name]
    assert disjoint_rule(shapes) == (groups, exps, max(groups) + 1)
    assert walk_disjoint(shapes) == (groups, exps, max(groups) + 1)


@pytest.mark.parametrize("name", ["mixed", "padtrim", "same_R", "forty"])
def test_plan_instances(oracle, name):
    nvs, rl = pc.instance_cases()[name]
    terms, groups = check_plan(nvs, rl, True)
    want = {"mixed": ([0, 1, 2, 3, 0, 1, 2, 3], [0, 0, 0, 0, 1, 2, 3, 4]),
            "padtrim": ([0, 0, 0], [0, 1, 2]),
            "same_R": ([0, 0, 1], [0, 1, 0]),
            "forty": ([i % 5 for i in range(40)], [0] * 5 + list(range(1, 36)))}[name]
    assert ([t[0] for t in terms], [t[1] for t in terms]) == want
