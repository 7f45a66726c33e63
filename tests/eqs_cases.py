"""Shared inputs of the short-sum tests (tests/test_gpu_eqs.py on the device through spg_eqs_check, tests/test_eqs_host.py
through libspg_hostcheck.so's host evaluation): calls of E equations over points from gens_stream(b"vmsm_test", 4096)
(vmsm_cases.points), every operand form, edge scalars, edge points and rejected encodings. The reference of an equation
is the oracle's orc_msm (pyoracle.msm) over the encodings of its terms' points, computed once per call and kept; the
expected status is 0 where that sum is the 32 zero bytes of the identity, else 1, and 2 for an equation that holds a
rejected encoding."""
import numpy as np

import fieldref
import vmsm_cases as vc

COMPRESSED, EXTENDED, INDEX = 0, 1, 2  # the operand forms of include/spg.h
NBASE = 16                             # the base handle: the first 16 points
LENGTHS = [0, 1, 2, 3, 4, 5, 22, 63, 64, 65, 257]
Q = fieldref.Q

_REF = {}


def base_points(oracle):
    return vc.points(oracle)[:NBASE]


def mont(v):
    return fieldref.arr_u64([fieldref.to_mont(v % Q)])[0]


def ext_bytes(enc, z=1, lift=()):
    """the 128-byte extended form (X, Y, Z, T little-endian) of the point an encoding names, scaled by z"""
    pt = fieldref.decode(bytes(enc))
    assert pt is not None
    return np.array(fieldref.ext_raw(pt, z, lift), dtype=np.uint32).tobytes()


class Call:
    """one spg_eqs_check call under construction: eq() opens an equation, term() appends to the open one"""

    def __init__(self, name):
        self.name = name
        self.forms, self.operands, self.scalars, self.first = [], [], [], [0]
        self.comp, self.ext = [], []
        self.encs = []      # per term: the encoding of its point (the oracle's input)
        self.invalid = []   # terms whose encoding DECODE rejects

    def eq(self):
        self.first.append(self.first[-1])
        return self

    def term(self, form, enc, scalar, z=1, lift=(), index=None, valid=True):
        enc = bytes(enc)
        if form == COMPRESSED:
            self.operands.append(len(self.comp))
            self.comp.append(np.frombuffer(enc, np.uint8))
        elif form == EXTENDED:
            self.operands.append(len(self.ext))
            self.ext.append(np.frombuffer(ext_bytes(enc, z, lift), np.uint8))
        else:
            self.operands.append(index)
        if not valid:
            self.invalid.append(len(self.forms))
        self.forms.append(form)
        self.scalars.append(np.asarray(scalar, np.uint64))
        self.encs.append(enc)
        self.first[-1] += 1
        return self

    @property
    def E(self):
        return len(self.first) - 1

    def arrays(self):
        """(forms, operands, scalars, first, compressed, extended) for spg.eqs_pack / spg.eqs_check"""
        s = np.array(self.scalars, np.uint64).reshape(-1, 4)
        comp = np.array(self.comp, np.uint8).reshape(-1, 32)
        ext = np.array(self.ext, np.uint8).reshape(-1, 128)
        return self.forms, self.operands, s, self.first, comp, ext

    def expected(self, oracle):
        """(status list, sums list (None where the status is 2), lowest rejected term or -1), once per call"""
        if self.name not in _REF:
            status, sums = [], []
            for e in range(self.E):
                t0, t1 = self.first[e], self.first[e + 1]
                if any(t0 <= t < t1 for t in self.invalid):
                    status.append(2)
                    sums.append(None)
                    continue
                ref = bytes(32)
                if t1 > t0:
                    ref = oracle.msm(np.frombuffer(b"".join(self.encs[t0:t1]), np.uint8).reshape(-1, 32),
                                     np.array(self.scalars[t0:t1], np.uint64))
                status.append(0 if ref == bytes(32) else 1)
                sums.append(ref)
            _REF[self.name] = (status, sums, min(self.invalid) if self.invalid else -1)
        return _REF[self.name]

    def check(self, oracle, status, sums, bad):
        want_status, want_sums, want_bad = self.expected(oracle)
        assert list(status) == want_status, (self.name, list(status), want_status)
        assert bad == want_bad, (self.name, bad, want_bad)
        if sums is not None:
            for e, w in enumerate(want_sums):
                assert bytes(sums[e]) == (w if w is not None else bytes(32)), (self.name, e)


def mixed_term(oracle, call, j, scalar):
    """term j of a generic equation: the forms in turn, points walking through the stream"""
    P = vc.points(oracle)
    form = j % 3
    if form == INDEX:
        call.term(INDEX, P[j % NBASE], scalar, index=j % NBASE)
    else:
        call.term(form, P[(7 * j + 3) % 4096], scalar, z=2 + j)


def lengths_call(oracle, name, lengths, seed):
    c = Call(name)
    s = vc.rand_fq(oracle, np.random.default_rng(seed), sum(lengths))
    k = 0
    for n in lengths:
        c.eq()
        for j in range(n):
            mixed_term(oracle, c, k, s[k])
            k += 1
    return c


def count_call(oracle, E):
    return lengths_call(oracle, "count_%d" % E, [5] * E, 1000 + E)


def scalar_call(oracle):
    """one equation of 5 terms per edge scalar, one with a random scalar repeated, one with the recode carry patterns"""
    c = Call("edge_scalars")
    rnd = vc.rand_fq(oracle, np.random.default_rng(5), 1)[0]
    for s in (mont(0), mont(1), mont(Q - 1), mont(2**252), rnd):
        c.eq()
        for j in range(5):
            mixed_term(oracle, c, j, s)
    c.eq()
    for j, v in enumerate(fieldref.api_carry_scalars()):
        mixed_term(oracle, c, j, mont(v))
    return c


def point_call(oracle):
    P = vc.points(oracle)
    rng = np.random.default_rng(77)
    s = vc.rand_fq(oracle, rng, 64)
    same = s[0]
    c = Call("edge_points")
    c.eq()  # the identity encoding among other points, compressed and extended
    for j in range(6):
        c.term(COMPRESSED, bytes(32) if j in (1, 5) else P[20 + j], s[j])
    c.term(EXTENDED, bytes(32), s[7], z=3)
    c.eq()  # P next to -P with equal scalars: the identity
    for j in range(4):
        c.term(COMPRESSED, P[30 + j], same)
        c.term(COMPRESSED if j % 2 else EXTENDED, vc.neg_point(oracle, P[30 + j]), same, z=5)
    c.eq()  # one point 64 times
    for j in range(64):
        c.term(COMPRESSED, P[7], same)
    c.eq()  # the same point in all three forms
    c.term(COMPRESSED, P[3], s[1]).term(EXTENDED, P[3], s[2]).term(INDEX, P[3], s[3], index=3)
    c.eq()  # extended operands with Z != 1 and coordinates at or above p
    c.term(EXTENDED, P[40], s[4], z=0x1234567).term(EXTENDED, P[41], s[5], z=Q, lift=("X", "Y", "Z", "T"))
    c.term(EXTENDED, P[42], s[6], z=fieldref.P - 1, lift=("T",))
    c.eq()  # s P - s P in two forms of one point
    c.term(INDEX, P[2], same, index=2).term(EXTENDED, P[2], mont(Q - fieldref.from_mont(fieldref.ints(same)[0])), z=9)
    return c


def rejected_encodings(n=6):
    """n encodings DECODE rejects, one per reason first (fieldref.decode_candidates)"""
    out, seen = [], set()
    cands = fieldref.decode_candidates(np.random.default_rng(11))
    for b in cands:
        why = fieldref.decode_why(b)[1]
        if why and why not in seen:
            seen.add(why)
            out.append(b)
    for b in cands:
        if len(out) >= n:
            break
        if fieldref.decode_why(b)[1] and b not in out:
            out.append(b)
    assert len(out) >= n and len(seen) >= 4, sorted(seen)
    return out[:n]


def invalid_call(oracle, where):
    """8 equations of 9 terms; equations 2 and 5 hold a rejected encoding at term `where` (0, 4 or 8), equation 6 two"""
    P = vc.points(oracle)
    bad = rejected_encodings()
    s = vc.rand_fq(oracle, np.random.default_rng(200 + where), 72)
    c = Call("invalid_at_%d" % where)
    k = 0
    for e in range(8):
        c.eq()
        for j in range(9):
            hit = (e in (2, 5) and j == where) or (e == 6 and j in (where, (where + 3) % 9))
            if hit:
                c.term(COMPRESSED, bad[(e + j) % len(bad)], s[k], valid=False)
            else:
                mixed_term(oracle, c, k, s[k])
            k += 1
    return c


def calls(oracle):
    out = [lengths_call(oracle, "lengths", LENGTHS, 1), lengths_call(oracle, "lengths_reversed", LENGTHS[::-1], 2)]
    out += [count_call(oracle, E) for E in (1, 64, 65, 300)]
    out += [scalar_call(oracle), point_call(oracle)]
    out += [invalid_call(oracle, w) for w in (0, 4, 8)]
    return {c.name: c for c in out}


NAMES = ["lengths", "lengths_reversed", "count_1", "count_64", "count_65", "count_300", "edge_scalars", "edge_points",
         "invalid_at_0", "invalid_at_4", "invalid_at_8"]

_CALLS = None


def get(oracle, name):
    global _CALLS
    if _CALLS is None:
        _CALLS = calls(oracle)
        assert sorted(_CALLS) == sorted(NAMES)
    return _CALLS[name]


def bad_argument_cases(oracle):
    """name -> keyword arguments of spg.eqs_pack that the argument check must refuse"""
    P = vc.points(oracle)
    s = vc.rand_fq(oracle, np.random.default_rng(9), 4)
    ok = dict(forms=[COMPRESSED, EXTENDED, INDEX, COMPRESSED], operands=[0, 0, 1, 1], scalars=s, first=[0, 2, 4],
              compressed=P[:2], extended=np.frombuffer(ext_bytes(P[5]), np.uint8))
    cases = {
        "first_decreasing": dict(ok, first=[0, 3, 2, 4]),
        "first_not_from_zero": dict(ok, first=[1, 2, 4]),
        "compressed_index_past_pool": dict(ok, operands=[2, 0, 1, 1]),
        "extended_index_past_pool": dict(ok, operands=[0, 1, 1, 1]),
        "base_index_past_handle": dict(ok, operands=[0, 0, NBASE, 1]),
        "unknown_form": dict(ok, forms=[COMPRESSED, 3, INDEX, COMPRESSED]),
    }
    return ok, cases
