"""CPU checks of the disjoint-rounds and univariate PolyEvalProof entries (include/spg.h spg_pe_*): the entry points
are declared and exported, the tests' checker (tests/polyeval_forms_ref.py over the oracle's headers) proves on every
shared case what the oracle's own verifiers accept, the product's plans (csrc/pe_plan.hpp through spgh_pe_plan_disjoint
and spgh_pe_plan_uni) follow the reference's rules stated in plain Python, and the checker's univariate evaluation is
the plain-integer sum."""
import ctypes
import os
import re

import numpy as np
import pytest

import fieldref as fr
import polyeval_cases as pc
import polyeval_forms_cases as fc
import polyeval_forms_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg.so")
HOSTCHECK = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg_hostcheck.so")
HDR = os.path.join(ROOT, "include", "spg.h")

PE_SYMBOLS = ["spg_pe_prove_disjoint", "spg_pe_verify_disjoint", "spg_pe_uni_evals", "spg_pe_prove_uni",
              "spg_pe_verify_uni"]
LABEL, TLABEL = b"gens_polyeval_test", b"polyeval_test"


@pytest.fixture(scope="module")
def seed(oracle):
    import workload

    return workload.tape_seed()


def test_pe_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(spg_[a-z0-9_]+)\s*\(", src))
    assert not [s for s in PE_SYMBOLS if s not in declared]
    assert sorted(s for s in declared if s.startswith("spg_pe_")) == sorted(PE_SYMBOLS)
    assert not [s for s in PE_SYMBOLS if s.startswith("spg_poly_")]
    lib = ctypes.CDLL(LIB)
    assert not [s for s in PE_SYMBOLS if not hasattr(lib, s)]


# ---------------------------------------------------------------- the checker on the shared cases
@pytest.mark.parametrize("name", list(fc.DISJOINT_CASES))
def test_checker_disjoint_verifies(oracle, seed, name):
    shapes, rq, ry, Zs = fc.disjoint_inputs(name)
    Zr = fc.disjoint_evals(shapes, rq, ry, Zs)
    gnv = fc.gens_nv(max(fc.lg(p * q) for p, q in shapes))
    good = ref.prove_disjoint(LABEL, gnv, TLABEL, seed, Zs, shapes, rq, ry, Zr)
    assert good.verified and good.nproofs == fc.DISJOINT_CASES[name][3]
    if name == "abacba":  # a wrong evaluation is not accepted
        Zr[2] = pc.scalars(2, 1)[0]
        assert not ref.prove_disjoint(LABEL, gnv, TLABEL, seed, Zs, shapes, rq, ry, Zr).verified


@pytest.mark.parametrize("name", list(fc.UNI_CASES))
def test_checker_uni_verifies(oracle, seed, name):
    nvs, r, Zs = fc.uni_inputs(name)
    Zr = ref.uni_evals(Zs, nvs, r)
    gnv = fc.gens_nv(max(nvs))
    good = ref.prove_uni(LABEL, gnv, TLABEL, seed, Zs, nvs, r, Zr)
    R_size = 1 << (max(nvs) - max(nvs) // 2)
    assert good.verified and len(good.proof) == fc.proof_bytes(R_size)
    if name == "ragged":
        Zr[5] = pc.scalars(2, 1)[0]
        assert not ref.prove_uni(LABEL, gnv, TLABEL, seed, Zs, nvs, r, Zr).verified


def test_checker_uni_evaluation_is_the_integer_sum(oracle):
    nvs, r, Zs = fc.uni_inputs("ragged")
    x = fr.from_mont(fr.ints(r)[0])
    got = [fr.from_mont(v) for v in fr.ints(ref.uni_evals(Zs, nvs, r))]
    want = [sum(fr.from_mont(z) * pow(x, k, fr.Q) for k, z in enumerate(fr.ints(Z))) % fr.Q for Z in Zs]
    assert got == want
    # at r = 0 the constant coefficient, at r = 1 the sum of all coefficients
    for name, pick in (("ragged_r0", lambda z: z[0]), ("ragged_r1", lambda z: sum(z) % fr.Q)):
        nvs, r, Zs = fc.uni_inputs(name)
        got = [fr.from_mont(v) for v in fr.ints(ref.uni_evals(Zs, nvs, r))]
        assert got == [pick([fr.from_mont(z) for z in fr.ints(Z)]) for Z in Zs]


# ---------------------------------------------------------------- the product's plans
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


def plan_disjoint(shapes, rq, ry):
    hc = ctypes.CDLL(HOSTCHECK)
    hc.spgh_pe_plan_disjoint.restype = ctypes.c_long
    n = len(shapes)
    term = (ctypes.c_size_t * (6 * n))()
    grp = (ctypes.c_size_t * (7 * n))()
    tot = (ctypes.c_size_t * 4)()
    nvs = [fc.lg(p * q) for p, q in shapes]
    fitted = np.zeros((sum(nvs), 4), np.uint64)
    flat = (ctypes.c_size_t * (2 * n))(*[x for s in shapes for x in s])
    q = np.ascontiguousarray(np.concatenate([rq, np.zeros((1, 4), np.uint64)]))
    y = np.ascontiguousarray(np.concatenate([ry, np.zeros((1, 4), np.uint64)]))
    k = hc.spgh_pe_plan_disjoint(ctypes.c_size_t(n), flat, q.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(rq)),
                                 y.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(ry)), term,
                                 fitted.ctypes.data_as(ctypes.c_void_p), grp, tot)
    terms = [tuple(term[6 * i:6 * i + 6]) for i in range(n)]
    groups = [tuple(grp[7 * g:7 * g + 7]) for g in range(k)]
    return terms, groups, fitted, tuple(tot)


@pytest.mark.parametrize("name", list(fc.DISJOINT_CASES))
def test_plan_disjoint(oracle, name):
    shapes, rq, ry, _ = fc.disjoint_inputs(name)
    g, e, k = disjoint_rule(shapes)
    terms, groups, fitted, (part_len, out_len, xblocks, nbytes) = plan_disjoint(shapes, rq, ry)
    assert len(groups) == k == fc.DISJOINT_CASES[name][3]
    assert [t[0] for t in terms] == g and [t[1] for t in terms] == e
    if name == "abacba":
        assert (g, e) == (fc.ABACBA_GROUPS, fc.ABACBA_EXPS)
    if name == "forty":
        assert e == [0] * 5 + list(range(1, 36))
    # fitted points: the reference's slice of rq, then ry padded at the front or trimmed from the front
    want = np.concatenate([fc.disjoint_point(s, rq, ry) for s in shapes])
    assert np.array_equal(fitted, want)
    if name == "abacba":
        p116 = fitted[6 + 4 + 6:6 + 4 + 6 + 4]  # (1, 16): no rq entry, one zero in front of the three ry entries
        assert not p116[0].any() and np.array_equal(p116[1:], ry)
        p44 = fitted[6:10]  # (4, 4): the last two of rq, the last two of ry
        assert np.array_equal(p44, np.concatenate([rq[1:], ry[1:]]))
    # groups in first-seen order with the key's shapes; every term is bound and covers its rows; slabs contiguous
    po = oo = 0
    for gi, (nv, Ls, Rs, first, S, part_off, out_off) in enumerate(groups):
        assert first == g.index(gi) and nv == fc.lg(shapes[first][0] * shapes[first][1])
        assert Ls == 1 << (nv // 2) and Rs == 1 << (nv - nv // 2)
        assert (part_off, out_off) == (po, oo)
        slab = 0
        for t in [t for t in terms if t[0] == gi]:
            assert t[2] == 1 and t[5] == slab and t[3] >= 1 and (t[3] - 1) * t[4] < Ls <= t[3] * t[4]
            slab += t[3]
        assert slab == S
        po, oo = po + S * Rs, oo + Rs
    assert (part_len, out_len) == (po, oo)
    assert xblocks == sum((groups[t[0]][2] + 255) // 256 for t in terms)
    assert nbytes == 8 + sum(fc.proof_bytes(Rs) for (_, _, Rs, *_) in groups)


def plan_uni(nvs, per_term, r=None, c_base=None):
    hc = ctypes.CDLL(HOSTCHECK)
    hc.spgh_pe_plan_uni.restype = ctypes.c_long
    n = len(nvs)
    term = (ctypes.c_size_t * (8 * n))()
    tot = (ctypes.c_size_t * 5)()
    ends = np.zeros((n, 2, 4), np.uint64)
    args = [None, None, None]
    if r is not None:
        r, c_base = np.ascontiguousarray(r, np.uint64), np.ascontiguousarray(c_base, np.uint64)
        args = [a.ctypes.data_as(ctypes.c_void_p) for a in (r, c_base, ends)]
    k = hc.spgh_pe_plan_uni(ctypes.c_int(1 if per_term else 0), ctypes.c_size_t(n), (ctypes.c_size_t * n)(*nvs), term,
                            tot, *args)
    assert k == n
    return [tuple(term[8 * i:8 * i + 8]) for i in range(n)], tuple(tot), ends


@pytest.mark.parametrize("per_term", [False, True])
@pytest.mark.parametrize("name", list(fc.UNI_CASES))
def test_plan_uni(name, per_term):
    nvs = fc.UNI_CASES[name][0]
    terms, (part_len, out_len, xblocks, nbytes, R_size), _ = plan_uni(nvs, per_term)
    assert R_size == max(1 << (nv - nv // 2) for nv in nvs) and nbytes == fc.proof_bytes(R_size)
    spans, oo = [], 0
    for i, (exp, nv, Ls, Rs, S, chunk, part_off, out_off) in enumerate(terms):
        assert exp == i and nv == nvs[i] and Ls == 1 << (nv // 2) and Rs == 1 << (nv - nv // 2)
        assert S >= 1 and S * chunk >= Ls > (S - 1) * chunk
        assert part_off + S * Rs <= part_len
        spans.append((part_off, part_off + S * Rs))
        assert out_off == (oo if per_term else 0)
        oo += Rs
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))  # slabs of different terms are disjoint
    assert part_len == sum(b - a for a, b in spans)
    assert xblocks == sum(((1 << (nv - nv // 2)) + 255) // 256 for nv in nvs)
    assert out_len == (oo if per_term else R_size)


def test_plan_uni_coefficients(oracle):
    """term i joins with c_base^i, the first with c^0: the first and last entries of its scaled table are c^i and
    c^i r^(Rs_i (Ls_i - 1)) over plain integers"""
    nvs, r, _ = fc.uni_inputs("ragged")
    c_base = pc.scalars(77, 1)[0]
    terms, _, ends = plan_uni(nvs, False, r, c_base)
    x, c = fr.from_mont(fr.ints(r)[0]), fr.from_mont(fr.ints(c_base)[0])
    for i, (exp, nv, Ls, Rs, *_) in enumerate(terms):
        first, last = (fr.from_mont(v) for v in fr.ints(ends[i]))
        assert first == pow(c, i, fr.Q) and last == pow(c, i, fr.Q) * pow(x, Rs * (Ls - 1), fr.Q) % fr.Q
