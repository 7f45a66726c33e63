"""ctypes binding of libspg.so — the MI355X-native Spartan prover hot path (C-ABI in include/spg.h).

Mirrors the reference crate's seams with the same argument meaning:
  * Gens(n, label)            ~ MultiCommitGens::new(n, label)          (src/commitments.rs:15-33)
  * Gens.msm(scalars, blind)  ~ GroupElement::vartime_multiscalar_mul   (src/group.rs:98-116)
                                + blind * h                              (src/commitments.rs:87-92)
  * Gens.commit_rows(Z, L, R) ~ DensePolynomial::commit_inner           (src/dense_mlpoly.rs:184-212)
Scalars are numpy uint64 arrays of shape (..., 4): the reference's Montgomery limbs.
There is no CPU fallback: constructing a Context without a gfx950 device raises.

The C signature of every spg_* function is read from include/spg.h when the library is loaded (_signatures, _bind):
callers pass plain Python ints for size_t / int / long arguments, and a wrong type stops in ctypes.
"""
import collections
import ctypes
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPG_LIB") or os.path.join(_HERE, "lib", "libspg.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "spg.h")

SPG_ERRORS = {-1: "SPG_E_ARG", -2: "SPG_E_NOMEM", -3: "SPG_E_HIP", -4: "SPG_E_POINT", -5: "SPG_E_NODEVICE",
              -6: "SPG_E_VERIFY", -7: "SPG_E_CALLBACK", -8: "SPG_E_UNSAT"}
SPG_E_VERIFY = -6
SPG_E_ARG = -1
SPG_E_UNSAT = -8

# by-value C types of the header; every parameter with a `*` or `[` is a pointer (c_void_p: handles, byref(), ctypes
# arrays, None, _p(numpy) and CFUNCTYPE thunks all pass), as are the callback typedefs
_C_VALUES = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double,
             "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
_C_CALLBACKS = ("spg_allgather_fn", "spg_transcript_append_fn", "spg_transcript_challenge_fn")
_PROTOTYPE = re.compile(r"^([A-Za-z_][\w \t*]*?)\s*\b(spg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.M)


def _signatures(text):
    """{name: (restype, [argtypes])} of every `<ret> spg_name(<params>);` prototype in header text; a type outside the
    table above raises, naming the function and the parameter"""
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(re.sub(r"/\*.*?\*/", "", text, flags=re.S)):
        ret = " ".join(ret.split())
        if ret == "const char*":
            restype = ctypes.c_char_p
        elif ret in _C_VALUES:
            restype = _C_VALUES[ret]
        else:
            raise ValueError(f"spg.h: {name}: return type '{ret}' has no ctypes mapping")
        argtypes = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in param.split() if w != "const"]
            ctype = " ".join(words[:-1])  # the last word is the parameter's name
            if "*" in param or "[" in param or ctype in _C_CALLBACKS:
                argtypes.append(ctypes.c_void_p)
            elif ctype in _C_VALUES:
                argtypes.append(_C_VALUES[ctype])
            else:
                raise ValueError(f"spg.h: {name}: parameter '{' '.join(param.split())}' has no ctypes mapping")
        sigs[name] = (restype, argtypes)
    return sigs


def _bind(cdll):
    """restype and argtypes of every function include/spg.h declares (a symbol the library lacks raises)"""
    with open(HEADER_PATH) as f:
        sigs = _signatures(f.read())
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libspg.so not built at {LIB_PATH}; run __graft_entry__.build()")
        cdll = ctypes.CDLL(LIB_PATH)
        _bind(cdll)
        _lib = cdll
    return _lib


def comb_stats():
    """spg_comb_stats: (HBM bytes of this process's comb tables now allocated, comb tables built so far, their summed
    build seconds, HBM bytes of the live generator sets' 2^k G_i tables) -- the fixed-base precomputation behind the MSM
    paths"""
    b = ctypes.c_uint64()
    k = ctypes.c_int()
    s = ctypes.c_double()
    g = ctypes.c_uint64()
    rc = lib().spg_comb_stats(ctypes.byref(b), ctypes.byref(k), ctypes.byref(s), ctypes.byref(g))
    if rc != 0:
        raise SpgError(f"spg_comb_stats: {SPG_ERRORS.get(rc, rc)}")
    return int(b.value), int(k.value), float(s.value), int(g.value)


_hc = None


def hostcheck():
    """lib/libspg_hostcheck.so: the host build of the product's field / curve / transcript code (tests, and the
    caller-side merlin of Transcript.from_native_merlin)"""
    global _hc
    if _hc is None:
        path = os.environ.get("SPG_HOSTCHECK_LIB") or os.path.join(_HERE, "lib", "libspg_hostcheck.so")
        _hc = ctypes.CDLL(path)
        _hc.spgh_merlin_new.restype = ctypes.c_void_p
        _hc.spgh_merlin_new.argtypes = [ctypes.c_char_p]
        _hc.spgh_merlin_free.argtypes = [ctypes.c_void_p]
        _hc.spgh_merlin_challenge_cb.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    return _hc


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class SpgError(RuntimeError):
    pass


# int (*spg_allgather_fn)(void* user, const void* send, size_t bytes, void* recv)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


def torch_allgather(dist, group=None, device="cpu"):
    """An spg_allgather_fn over torch.distributed (gloo: device='cpu'; nccl = RCCL: device='cuda:<local>'):
    the `bytes` of rank k land at recv + k * bytes on every rank."""
    import torch

    def cb(user, send, nbytes, recv):
        try:
            world = dist.get_world_size(group)
            buf = bytearray(ctypes.string_at(send, nbytes)) if nbytes else bytearray(1)
            src = torch.frombuffer(buf, dtype=torch.uint8).to(device)
            outs = [torch.empty_like(src) for _ in range(world)]
            dist.all_gather(outs, src, group=group)
            flat = torch.cat(outs).cpu().numpy() if nbytes else None
            if nbytes:
                for k in range(world):
                    ctypes.memmove(recv + k * nbytes, flat[k * len(buf):].ctypes.data, nbytes)
            return 0
        except Exception as e:  # noqa: BLE001 - reported through the return code
            import sys

            print(f"spg allgather callback failed: {e!r}", file=sys.stderr)
            return 1

    return ALLGATHER_FN(cb)


class Context:
    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        rc = lib().spg_init(device, ctypes.byref(self._h))
        if rc != 0:
            raise SpgError(f"spg_init({device}) failed: {SPG_ERRORS.get(rc, rc)} (no gfx950 device?)")

    def check(self, rc, what):
        if rc != 0:
            msg = lib().spg_last_error(self._h).decode(errors="replace")
            raise SpgError(f"{what}: {SPG_ERRORS.get(rc, rc)}: {msg}")

    def call(self, name, *args):
        """lib().<name>(this context, *args), its return code checked under that name"""
        self.check(getattr(lib(), name)(self._h, *args), name)

    def out_buf(self, cap):
        """the proof output buffer of this context's calls, kept between calls (a context runs one call at a time;
        each wrapper copies its bytes out): a fresh 16 MB np.zeros per prove cost ~0.3 ms of mmap / munmap and page
        faults beside the pool's spinning threads"""
        b = getattr(self, "_out", None)
        if b is None or b.shape[0] < cap:
            b = self._out = np.empty(cap, dtype=np.uint8)
        return b

    @property
    def handle(self):
        return self._h

    def set_comm(self, rank, nranks, allgather_fn=None):
        """spg_set_comm: shard R1CSProof::prove by instance over nranks processes (one GPU each)."""
        self._comm = allgather_fn  # keep the ctypes thunk alive
        self.call("spg_set_comm", rank, nranks, allgather_fn, None)

    def set_comm_rccl(self, rank, nranks, dist=None, unique_id=None):
        """spg_set_comm_rccl: libspg's own RCCL transport on the context stream. Rank 0's 128-byte id
        (spg_rccl_unique_id) reaches every rank through `dist` (torch.distributed broadcast_object_list over the
        default group) unless unique_id is given."""
        if unique_id is None:
            buf = (ctypes.c_uint8 * 128)()
            if rank == 0:
                rc = lib().spg_rccl_unique_id(buf)
                if rc != 0:
                    raise SpgError(f"spg_rccl_unique_id: {SPG_ERRORS.get(rc, rc)}")
            if nranks > 1:
                obj = [bytes(buf) if rank == 0 else None]
                dist.broadcast_object_list(obj, src=0)
                unique_id = obj[0]
            else:
                unique_id = bytes(buf)
        uid = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        self._comm = None
        self.call("spg_set_comm_rccl", uid, rank, nranks)

    def comm_allgather(self, data, nranks):
        """spg_comm_allgather over the context's transport: every rank's `data` (equal lengths), rank-ordered"""
        n = len(data)
        src = (ctypes.c_uint8 * max(n, 1)).from_buffer_copy(bytes(data) or b"\0")
        dst = (ctypes.c_uint8 * max(n * nranks, 1))()
        self.call("spg_comm_allgather", src, n, dst)
        raw = bytes(dst)
        return [raw[k * n:(k + 1) * n] for k in range(nranks)]

    def set_comb(self, on=True):
        """spg_set_comb: off -> this context's MSMs skip the comb tables (bucket Pippenger pipelines only)"""
        self.call("spg_set_comb", 1 if on else 0)

    def set_vmsm_host_max(self, n=-1):
        """spg_set_vmsm_host_max: this context's variable-base MSMs of fewer than n points run on the host pool (0:
        every size through the kernels; negative: the process default)"""
        self.call("spg_set_vmsm_host_max", n)

    def set_verify_device(self, on=True):
        """spg_set_verify_device: this context's verifiers collect their sigma-protocol group equations and check them
        in one spg_eqs_check launch at the end of the call (same verdicts and error texts; off by default)"""
        self.call("spg_set_verify_device", 1 if on else 0)

    def set_check_sat(self, on=True):
        """spg_set_check_sat: spg_r1cs_prove (and through it spg_snark_prove) checks Az * Bz == Cz on the device right
        after its multiply_vec_block and refuses an unsatisfying witness with SPG_E_UNSAT, naming the row"""
        self.call("spg_set_check_sat", 1 if on else 0)

    def eqs_last_counts(self):
        """spg_eqs_last_counts: (equations, terms) of this context's most recent spg_eqs_check launch, a deferred
        verifier's included"""
        e, t = ctypes.c_size_t(), ctypes.c_size_t()
        self.call("spg_eqs_last_counts", ctypes.byref(e), ctypes.byref(t))
        return int(e.value), int(t.value)

    def last_kernel_us(self):
        return lib().spg_last_kernel_us(self._h)

    def prof_enable(self, on=True):
        self.call("spg_prof_enable", 1 if on else 0)

    def prof_read(self, reset=True, ops=False):
        """{kernel_name: (launches, total_us, algorithmic_bytes)} of the kernels timed since the last reset;
        ops=True appends the modelled VALU work of those launches to each tuple: curve mixed additions, then Fq
        products."""
        mx = 128
        names = ctypes.create_string_buffer(32 * mx)
        launches = np.zeros(mx, dtype=np.int64)
        tot = np.zeros(mx, dtype=np.float64)
        nbytes = np.zeros(mx, dtype=np.float64)
        nops = np.zeros(mx, dtype=np.float64)
        nfqm = np.zeros(mx, dtype=np.float64)
        k = lib().spg_prof_read3(self._h, names, _p(launches), _p(tot), _p(nbytes), _p(nops), _p(nfqm), mx,
                                 1 if reset else 0)
        if k < 0:
            self.check(k, "spg_prof_read3")
        raw = names.raw
        out = {}
        for i in range(k):
            nm = raw[32 * i:32 * i + 32].split(b"\0", 1)[0].decode()
            rec = (int(launches[i]), float(tot[i]), float(nbytes[i]))
            out[nm] = rec + (float(nops[i]), float(nfqm[i])) if ops else rec
        return out

    def close(self):
        if self._h:
            lib().spg_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    """An object that owns one native handle (self._h; self.ctx where its free function takes the context): freed
    once, by free() or when the object is collected."""

    _free = None  # the name of the spg_*_free function

    @property
    def handle(self):
        return self._h

    def free(self):
        if self._h:
            fn = getattr(lib(), self._free)
            if len(fn.argtypes) == 2:
                fn(self.ctx.handle, self._h)
            else:
                fn(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _scalars(x):
    a = np.ascontiguousarray(x, dtype=np.uint64)
    if a.shape[-1] != 4:
        a = a.reshape(-1, 4)
    return a


class Buf(_Handle):
    """Device-resident vector of Montgomery scalars (spg_buf)."""

    _free = "spg_buf_free"

    def __init__(self, ctx, scalars):
        self.ctx = ctx
        a = _scalars(scalars)
        self.n = a.shape[0]
        self._h = ctypes.c_void_p()
        ctx.call("spg_buf_upload", _p(a), self.n, ctypes.byref(self._h))

    def download(self):
        out = np.zeros((self.n, 4), dtype=np.uint64)
        self.ctx.call("spg_buf_download", self._h, _p(out))
        return out

    @classmethod
    def eq_evals(cls, ctx, r):
        """EqPolynomial::new(r).evals() (src/dense_mlpoly.rs:76-92) built on the device (spg_eq_evals)."""
        a = _scalars(r) if len(r) else np.zeros((0, 4), dtype=np.uint64)
        b = cls.__new__(cls)
        b.ctx = ctx
        b.n = 1 << a.shape[0]
        b._h = ctypes.c_void_p()
        ctx.call("spg_eq_evals", _p(a), a.shape[0], ctypes.byref(b._h))
        return b

    # per-operation seams (csrc/seams.hip)
    def bound_top(self, r):
        """DensePolynomial::bound_poly_var_top (src/dense_mlpoly.rs:267-275), in place; the length halves."""
        self.ctx.call("spg_buf_bound_top", self._h, _p(_scalars(r)))
        self.n //= 2

    def bound_bot(self, r):
        """DensePolynomial::bound_poly_var_bot (src/dense_mlpoly.rs:350-358), in place; the length halves."""
        self.ctx.call("spg_buf_bound_bot", self._h, _p(_scalars(r)))
        self.n //= 2

    def evaluate(self, r):
        """DensePolynomial::evaluate (src/dense_mlpoly.rs:361-367) at r (len(r) = log2 of the length)."""
        a = _scalars(r) if len(r) else np.zeros((1, 4), dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self.ctx.call("spg_buf_evaluate", self._h, _p(a), len(r), _p(out))
        return out

    @staticmethod
    def cubic_round_evals(A, B, C):
        """One prove_cubic round's (e0, e2, e3) with comb A B C (src/sumcheck.rs:207-236)."""
        out = np.zeros((3, 4), dtype=np.uint64)
        A.ctx.call("spg_cubic_round_evals", A._h, B._h, C._h, _p(out))
        return out

    @staticmethod
    def prove_cubic(claim, num_rounds, A, B, C, transcript):
        """SumcheckInstanceProof::prove_cubic with comb A B C (src/sumcheck.rs:193-262): A, B, C bound in place.
        Returns (compressed polys [num_rounds, 3, 4], r [num_rounds, 4], claims [3, 4])."""
        polys = np.zeros((max(num_rounds, 1), 3, 4), dtype=np.uint64)
        r = np.zeros((max(num_rounds, 1), 4), dtype=np.uint64)
        claims = np.zeros((3, 4), dtype=np.uint64)
        A.ctx.call("spg_prove_cubic", _p(_scalars(claim)), num_rounds, A._h, B._h, C._h, transcript.handle, _p(polys),
                   _p(r), _p(claims))
        for b in (A, B, C):
            b.n >>= num_rounds
        return polys[:num_rounds], r[:num_rounds], claims


def _z_of_shape(z, num_proofs, num_witness_secs, num_inputs, what):
    """z as [n, 4] limbs, its length checked against the shape's total before native code reads that many scalars
    (a shorter array would be read past its end; whether the shape itself is valid is the native call's to say)"""
    a = _scalars(z)
    assert len(num_proofs) == len(num_inputs), f"{what}: num_proofs and num_inputs differ in length"
    total = sum(int(q) * int(num_witness_secs) * int(x) for q, x in zip(num_proofs, num_inputs))
    assert a.shape[0] >= total, f"{what}: z holds {a.shape[0]} scalars, the shape needs {total}"
    return a


def _pqx_from_handle(ctx, h, P, n):
    """a Pqx over a native handle of P instances and n allocated scalars"""
    t = Pqx.__new__(Pqx)
    t.ctx, t._h, t.P, t.n = ctx, h, P, n
    return t


class Pqx(_Handle):
    """DensePolynomialPqx (src/custom_dense_mlpoly.rs:22-359) resident in HBM (spg_pqx_*): z holds instance p's
    num_proofs[p] x num_witness_secs x num_inputs[p] scalars in (q_rev, w, x_rev) order, instances concatenated."""

    _free = "spg_pqx_free"

    def __init__(self, ctx, z, num_proofs, max_num_proofs, num_witness_secs, num_inputs, max_num_inputs):
        self.ctx = ctx
        a = _z_of_shape(z, num_proofs, num_witness_secs, num_inputs, "Pqx")
        self.P = len(num_proofs)
        self.n = a.shape[0]
        np_ = np.asarray(num_proofs, dtype=np.uint64)
        ni_ = np.asarray(num_inputs, dtype=np.uint64)
        self._h = ctypes.c_void_p()
        ctx.call("spg_pqx_new", _p(a), self.P, _p(np_), max_num_proofs, num_witness_secs, _p(ni_), max_num_inputs,
                 ctypes.byref(self._h))

    @classmethod
    def new_rev(cls, ctx, z, num_proofs, max_num_proofs, num_witness_secs, num_inputs, max_num_inputs, offset=0):
        """DensePolynomialPqx::new_rev (src/custom_dense_mlpoly.rs:67-111) of z in the standard (p, q, w, x) order,
        reordered on the device. z: host scalars (spg_pqx_new_rev), or a Buf read at `offset` with no host copy
        (spg_pqx_new_rev_buf)."""
        P = len(num_proofs)
        assert P == len(num_inputs), "Pqx.new_rev: num_proofs and num_inputs differ in length"
        np_ = np.asarray(num_proofs, dtype=np.uint64)
        ni_ = np.asarray(num_inputs, dtype=np.uint64)
        t = cls.__new__(cls)
        t.ctx, t.P, t._h = ctx, P, ctypes.c_void_p()
        t.n = sum(int(q) * int(num_witness_secs) * int(x) for q, x in zip(num_proofs, num_inputs))
        shape = (P, _p(np_), max_num_proofs, num_witness_secs, _p(ni_), max_num_inputs, ctypes.byref(t._h))
        if isinstance(z, Buf):
            ctx.call("spg_pqx_new_rev_buf", z.handle, offset, *shape)
        else:
            assert offset == 0, "Pqx.new_rev: offset is for a Buf"
            a = _z_of_shape(z, num_proofs, num_witness_secs, num_inputs, "Pqx.new_rev")
            ctx.call("spg_pqx_new_rev", _p(a), *shape)
        return t

    def bound_rq(self, rq):
        """bound_poly_vars_rq (src/custom_dense_mlpoly.rs:300-304): bound(rq[0], 2), bound(rq[1], 2), .. in order; one
        pass over the table for two or more challenges"""
        a = _scalars(rq) if len(rq) else np.zeros((1, 4), dtype=np.uint64)
        self.ctx.call("spg_pqx_bound_rq", self._h, _p(a), len(rq))

    def bound(self, r, mode):
        """bound_poly(r, mode): 1 = p, 2 = q, 3 = w, 4 = x (src/custom_dense_mlpoly.rs:180-199)"""
        self.ctx.call("spg_pqx_bound", self._h, _p(_scalars(r)), mode)

    def evaluate(self, rp, rq, rw, rx):
        """evaluate(r_p, r_q, r_w, r_x) (src/custom_dense_mlpoly.rs:320-333); the table is left unchanged"""
        arrs = [_scalars(r) if len(r) else np.zeros((1, 4), dtype=np.uint64) for r in (rp, rq, rw, rx)]
        args = []
        for a, r in zip(arrs, (rp, rq, rw, rx)):
            args += [_p(a), len(r)]
        out = np.zeros(4, dtype=np.uint64)
        self.ctx.call("spg_pqx_evaluate", self._h, *args, _p(out))
        return out

    def shape(self):
        dims = np.zeros(4, dtype=np.uint64)
        npf = np.zeros(self.P, dtype=np.uint64)
        nin = np.zeros(self.P, dtype=np.uint64)
        assert lib().spg_pqx_shape(self._h, _p(dims), _p(npf), _p(nin)) == 0
        return tuple(int(x) for x in dims), [int(x) for x in npf], [int(x) for x in nin]

    def download(self):
        out = np.zeros((self.n, 4), dtype=np.uint64)
        self.ctx.call("spg_pqx_download", self._h, _p(out))
        return out


class Gens(_Handle):
    """Device-resident MultiCommitGens (G_0..G_{n-1}, h) with fixed-base window tables."""

    _free = "spg_gens_free"

    def __init__(self, ctx, n, label=None, compressed=None):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        if compressed is not None:
            comp = np.ascontiguousarray(compressed, dtype=np.uint8).reshape(-1, 32)
            assert comp.shape[0] == n + 1
            ctx.call("spg_gens_upload", _p(comp), n, ctypes.byref(self._h))
        else:
            lb = np.frombuffer(bytes(label), dtype=np.uint8).copy() if label else np.zeros(1, np.uint8)
            ctx.call("spg_gens_derive", _p(lb), len(label or b""), n, ctypes.byref(self._h))
        self.n = n

    def compressed(self):
        out = np.zeros((self.n + 1, 32), dtype=np.uint8)
        self.ctx.call("spg_gens_download", self._h, _p(out))
        return out

    def msm(self, scalars, blind=None, gen_offset=0):
        s = _scalars(scalars)
        out = np.zeros(32, dtype=np.uint8)
        bl = None if blind is None else _scalars(blind)
        self.ctx.call("spg_msm", self._h, gen_offset, _p(s), s.shape[0], None if bl is None else _p(bl), _p(out))
        return out.tobytes()

    def msm_partial(self, scalars, gen_offset=0):
        """spg_msm_partial: uncompressed (X, Y, Z, T) partial sum of one shard, 128 bytes"""
        s = _scalars(scalars)
        out = np.zeros(128, dtype=np.uint8)
        self.ctx.call("spg_msm_partial", self._h, gen_offset, _p(s), s.shape[0], _p(out))
        return out.tobytes()

    def msm_partial_buf(self, buf, offset=0, n=None, gen_offset=0):
        """spg_msm_partial_buf: the partial sum of scalars already resident in HBM (a Buf), 128 bytes"""
        n = buf.n - offset if n is None else n
        out = np.zeros(128, dtype=np.uint8)
        self.ctx.call("spg_msm_partial_buf", self._h, gen_offset, buf._h, offset, n, _p(out))
        return out.tobytes()

    def msm_buf(self, buf, offset=0, n=None, gen_offset=0):
        """spg_msm_buf: vartime_multiscalar_mul of resident scalars, 32-byte compression"""
        n = buf.n - offset if n is None else n
        out = np.zeros(32, dtype=np.uint8)
        self.ctx.call("spg_msm_buf", self._h, gen_offset, buf._h, offset, n, _p(out))
        return out.tobytes()

    def commit_rows(self, Z, L, R, blinds=None):
        z = _scalars(Z)
        assert z.shape[0] == L * R
        out = np.zeros((L, 32), dtype=np.uint8)
        bl = None if blinds is None else _scalars(blinds)
        self.ctx.call("spg_commit_rows", self._h, _p(z), L, R, None if bl is None else _p(bl), _p(out))
        return out

    def commit_rows_buf(self, zbuf, L, R, offset=0, blinds_buf=None):
        out = np.zeros((L, 32), dtype=np.uint8)
        self.ctx.call("spg_commit_rows_buf", self._h, zbuf.handle, offset, L, R,
                      None if blinds_buf is None else blinds_buf.handle, _p(out))
        return out


class Points(_Handle):
    """Device-resident points a caller supplies (spg_points): n CompressedRistretto encodings kept as affine Niels, for
    GroupElement::vartime_multiscalar_mul over points that are no generator set (src/group.rs:98-116). An encoding
    that does not decompress raises SpgError (SPG_E_POINT, naming the lowest such index)."""

    _free = "spg_points_free"

    def __init__(self, ctx, compressed):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        comp = np.ascontiguousarray(compressed, dtype=np.uint8).reshape(-1, 32)
        ctx.call("spg_points_upload", _p(comp), comp.shape[0], ctypes.byref(self._h))
        self.n = int(lib().spg_points_n(self._h))

    def compressed(self):
        out = np.zeros((self.n, 32), dtype=np.uint8)
        self.ctx.call("spg_points_download", self._h, _p(out))
        return out

    def msm(self, scalars, offset=0):
        """spg_msm_var: sum_i scalars[i] * P[offset + i], 32-byte compression"""
        s = _scalars(scalars)
        out = np.zeros(32, dtype=np.uint8)
        self.ctx.call("spg_msm_var", self._h, offset, _p(s), s.shape[0], _p(out))
        return out.tobytes()

    def msm_buf(self, buf, offset=0, s_offset=0, n=None):
        """spg_msm_var_buf: the same over scalars resident in HBM (a Buf)"""
        n = buf.n - s_offset if n is None else n
        out = np.zeros(32, dtype=np.uint8)
        self.ctx.call("spg_msm_var_buf", self._h, offset, buf.handle, s_offset, n, _p(out))
        return out.tobytes()

    def msm_batch(self, offsets, lens, scalars):
        """spg_msm_var_batch: MSM b sums lens[b] points from offsets[b]; scalars concatenated in b order; (B, 32)"""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint64)
        assert offs.shape == ln.shape and offs.ndim == 1
        s = _scalars(scalars) if int(ln.sum()) else np.zeros((1, 4), dtype=np.uint64)
        assert int(ln.sum()) == 0 or s.shape[0] == int(ln.sum())
        out = np.zeros((offs.shape[0], 32), dtype=np.uint8)
        self.ctx.call("spg_msm_var_batch", self._h, _p(offs), _p(ln), offs.shape[0], _p(s), _p(out))
        return out


def msm_points(ctx, compressed, scalars):
    """spg_msm_points: vartime_multiscalar_mul(scalars, points) in one call (upload, sum, free)"""
    comp = np.ascontiguousarray(compressed, dtype=np.uint8).reshape(-1, 32)
    s = _scalars(scalars) if comp.shape[0] else np.zeros((0, 4), dtype=np.uint64)
    assert s.shape[0] == comp.shape[0]
    out = np.zeros(32, dtype=np.uint8)
    ctx.call("spg_msm_points", _p(comp), _p(s), comp.shape[0], _p(out))
    return out.tobytes()


# operand forms of spg_eqs_check (the header's SPG_EQS_* values)
EQS_COMPRESSED, EQS_EXTENDED, EQS_INDEX = 0, 1, 2


def eqs_pack(forms, operands, scalars, first, compressed=None, extended=None):
    """the flat arrays of one spg_eqs_check call: (compressed (nc, 32) u8, extended (ne, 128) u8, forms u8, operands
    u32, scalars (T, 4) u64, first u64 of E + 1 entries)"""
    comp = np.ascontiguousarray(np.zeros((0, 32), np.uint8) if compressed is None else compressed,
                                dtype=np.uint8).reshape(-1, 32)
    ext = np.ascontiguousarray(np.zeros((0, 128), np.uint8) if extended is None else extended,
                               dtype=np.uint8).reshape(-1, 128)
    f = np.ascontiguousarray(forms, dtype=np.uint8).reshape(-1)
    o = np.ascontiguousarray(operands, dtype=np.uint32).reshape(-1)
    s = _scalars(scalars) if f.shape[0] else np.zeros((0, 4), dtype=np.uint64)
    fi = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
    assert f.shape == o.shape and s.shape[0] == f.shape[0] and fi.shape[0] >= 1
    return comp, ext, f, o, s, fi


def eqs_check(ctx, forms, operands, scalars, first, compressed=None, extended=None, base=None, sums=True):
    """spg_eqs_check: E = len(first) - 1 sums of terms first[e] .. first[e + 1], term i = scalars[i] times the point
    operands[i] of the pool forms[i] names (EQS_COMPRESSED: compressed, EQS_EXTENDED: extended (128 bytes each),
    EQS_INDEX: the Points `base`). Returns (status u8[E]: 0 identity / 1 not / 2 rejected encoding, the (E, 32)
    encodings of the sums or None, the lowest rejected term or -1). Malformed arguments raise SpgError (SPG_E_ARG)."""
    comp, ext, f, o, s, fi = eqs_pack(forms, operands, scalars, first, compressed, extended)
    E = fi.shape[0] - 1
    status = np.full(max(E, 1), 255, dtype=np.uint8)
    out = np.zeros((max(E, 1), 32), dtype=np.uint8) if sums else None
    bad = ctypes.c_long(-2)
    ctx.call("spg_eqs_check", base.handle if base is not None else None, _p(comp) if comp.shape[0] else None,
             comp.shape[0], _p(ext) if ext.shape[0] else None, ext.shape[0], _p(f) if f.shape[0] else None,
             _p(o) if o.shape[0] else None, _p(s) if s.shape[0] else None, _p(fi), E,
             _p(out) if sums else None, _p(status), ctypes.byref(bad))
    return status[:E], (out[:E] if sums else None), int(bad.value)


# ---------------------------------------------------------------- Fiat-Shamir objects
# int (*spg_transcript_append_fn)(void* user, const char* label, const uint8_t* msg, size_t len)
# int (*spg_transcript_challenge_fn)(void* user, const char* label, uint8_t* out, size_t len)
TRANSCRIPT_APPEND_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t)
TRANSCRIPT_CHALLENGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p,
                                           ctypes.c_size_t)


class Transcript(_Handle):
    """ProofTranscript over merlin (src/transcript.rs:5-63), host object in libspg; or, with from_callbacks, a view
    of the caller's own transcript (every append_message / challenge_bytes is forwarded to it)."""

    _free = "spg_transcript_free"

    def __init__(self, label):
        self._h = ctypes.c_void_p()
        rc = lib().spg_transcript_new(bytes(label), ctypes.byref(self._h))
        if rc != 0:
            raise SpgError(f"spg_transcript_new: {SPG_ERRORS.get(rc, rc)}")

    @classmethod
    def from_callbacks(cls, append, challenge):
        """spg_transcript_new_callbacks: append(label: bytes, msg: bytes) and challenge(label: bytes, n) -> n bytes
        are the caller's merlin append_message / challenge_bytes; an exception in either is a failed callback
        (the running call returns SPG_E_CALLBACK)."""

        def app(user, label, msg, n):
            try:
                append(label, ctypes.string_at(msg, n) if n else b"")
                return 0
            except Exception:  # noqa: BLE001 - reported through the return code
                return 1

        def chal(user, label, out, n):
            try:
                b = challenge(label, n)
                assert len(b) == n
                if n:
                    ctypes.memmove(out, b, n)
                return 0
            except Exception:  # noqa: BLE001
                return 1

        t = cls.__new__(cls)
        t._cbs = (TRANSCRIPT_APPEND_FN(app), TRANSCRIPT_CHALLENGE_FN(chal))  # keep the thunks alive
        t._h = ctypes.c_void_p()
        rc = lib().spg_transcript_new_callbacks(t._cbs[0], t._cbs[1], None, ctypes.byref(t._h))
        if rc != 0:
            raise SpgError(f"spg_transcript_new_callbacks: {SPG_ERRORS.get(rc, rc)}")
        return t

    @classmethod
    def from_native_merlin(cls, label):
        """spg_transcript_new_callbacks over a caller-owned merlin::Transcript in native code (libspg_hostcheck's
        spgh_merlin_*: C callbacks, no Python per append / challenge) -- the drop-in mode a Rust caller gets with
        extern "C" trampolines over its &mut Transcript. The returned object also holds
        the caller's transcript: caller_challenge(label, n) reads challenge bytes from it after a prove."""
        hc = hostcheck()
        t = cls.__new__(cls)
        t._merlin = ctypes.c_void_p(hc.spgh_merlin_new(ctypes.c_char_p(bytes(label))))
        t._free_merlin = hc.spgh_merlin_free
        t._h = ctypes.c_void_p()
        rc = lib().spg_transcript_new_callbacks(ctypes.cast(hc.spgh_merlin_append_cb, ctypes.c_void_p),
                                                ctypes.cast(hc.spgh_merlin_challenge_cb, ctypes.c_void_p),
                                                t._merlin, ctypes.byref(t._h))
        if rc != 0:
            hc.spgh_merlin_free(t._merlin)
            raise SpgError(f"spg_transcript_new_callbacks: {SPG_ERRORS.get(rc, rc)}")
        return t

    def caller_challenge(self, label, n):
        out = (ctypes.c_uint8 * max(n, 1))()
        hostcheck().spgh_merlin_challenge_cb(self._merlin, bytes(label), out, n)
        return bytes(out)[:n]

    def append_message(self, label, msg):
        m = np.frombuffer(bytes(msg), dtype=np.uint8).copy() if msg else np.zeros(1, np.uint8)
        rc = lib().spg_transcript_append_message(self._h, bytes(label), _p(m), len(msg))
        if rc != 0:
            raise SpgError(f"spg_transcript_append_message: {SPG_ERRORS.get(rc, rc)}")

    def append_scalar(self, label, s):
        a = _scalars(s)
        assert lib().spg_transcript_append_scalar(self._h, bytes(label), _p(a)) == 0

    def challenge_scalar(self, label):
        out = np.zeros(4, dtype=np.uint64)
        assert lib().spg_transcript_challenge_scalar(self._h, bytes(label), _p(out)) == 0
        return out

    def challenge_bytes(self, label, n):
        out = np.zeros(max(n, 1), dtype=np.uint8)
        rc = lib().spg_transcript_challenge_bytes(self._h, bytes(label), _p(out), n)
        if rc != 0:
            raise SpgError(f"spg_transcript_challenge_bytes: {SPG_ERRORS.get(rc, rc)}")
        return out[:n].tobytes()

    def free(self):
        """the native transcript, then the caller-side merlin of from_native_merlin"""
        super().free()
        m = getattr(self, "_merlin", None)
        if m:
            self._free_merlin(m)
            self._merlin = None


class RandomTape(_Handle):
    """RandomTape (src/random.rs:7-29) with a caller-supplied init scalar (Montgomery limbs)."""

    _free = "spg_random_tape_free"

    def __init__(self, name, init_scalar):
        self._h = ctypes.c_void_p()
        a = _scalars(init_scalar)
        rc = lib().spg_random_tape_new(bytes(name), _p(a), ctypes.byref(self._h))
        if rc != 0:
            raise SpgError(f"spg_random_tape_new: {SPG_ERRORS.get(rc, rc)}")

    def random_scalar(self, label):
        out = np.zeros(4, dtype=np.uint64)
        assert lib().spg_random_tape_scalar(self._h, bytes(label), _p(out)) == 0
        return out


# ---------------------------------------------------------------- R1CSProof
class R1CSGens(_Handle):
    """R1CSGens::new(label, _, num_vars) (src/r1csproof.rs:71-79), resident in HBM."""

    _free = "spg_r1cs_gens_free"

    def __init__(self, ctx, label, num_vars):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        lb = np.frombuffer(bytes(label), dtype=np.uint8).copy()
        ctx.call("spg_r1cs_gens_new", _p(lb), len(label), num_vars, ctypes.byref(self._h))

    def compressed(self):
        cnt = ctypes.c_size_t(0)
        self.ctx.check(lib().spg_r1cs_gens_download(self.ctx.handle, self._h, None, ctypes.byref(cnt)), "download")
        out = np.zeros((cnt.value, 32), dtype=np.uint8)
        self.ctx.check(lib().spg_r1cs_gens_download(self.ctx.handle, self._h, _p(out), ctypes.byref(cnt)), "download")
        return out


class R1CSInst(_Handle):
    """R1CSInstance uploaded once (CSR + merged CSC in HBM). `cinst` is a workload.CViews().inst."""

    _free = "spg_r1cs_inst_free"

    def __init__(self, ctx, cinst):
        self.ctx = ctx
        self.num_instances = int(cinst.num_instances)  # the handle's own matrix count (1: shared by every instance)
        self._h = ctypes.c_void_p()
        ctx.call("spg_r1cs_inst_new", ctypes.byref(cinst), ctypes.byref(self._h))


def phase1_round_evals(Ap, Aq, Ax, B, C, D, mode):
    """one x (mode 4) or q (mode 2) round of the phase-1 sumcheck (src/sumcheck.rs:1173-1245): (e0, e2, e3)"""
    out = np.zeros((3, 4), dtype=np.uint64)
    Ap.ctx.call("spg_phase1_round_evals", Ap.handle, Aq.handle, Ax.handle, B._h, C._h, D._h, mode, _p(out))
    return out


def phase2_round_evals(A, ABC, Z, mode, single_inst, num_witness_secs):
    """one y (4), w (3) or p (1) round of the phase-2 sumcheck (src/sumcheck.rs:881-941): (e0, e2, e3)"""
    out = np.zeros((3, 4), dtype=np.uint64)
    A.ctx.call("spg_phase2_round_evals", A.handle, ABC._h, Z._h, mode, 1 if single_inst else 0, num_witness_secs,
               _p(out))
    return out


def r1cs_multiply_vec_block(ctx, inst, num_proofs, max_num_proofs, num_inputs, max_num_inputs, num_witness_secs, z):
    """R1CSInstance::multiply_vec_block (src/r1csinstance.rs:363-436) -> (Az, Bz, Cz) as resident Pqx tables; z holds
    instance p's num_proofs[p] x num_witness_secs x num_inputs[p] scalars, instances concatenated"""
    P = len(num_proofs)
    a = _z_of_shape(z, num_proofs, num_witness_secs, num_inputs, "r1cs_multiply_vec_block")
    np_ = np.asarray(num_proofs, dtype=np.uint64)
    ni_ = np.asarray(num_inputs, dtype=np.uint64)
    hs = [ctypes.c_void_p() for _ in range(3)]
    ctx.call("spg_r1cs_multiply_vec_block", inst.handle, P, _p(np_), max_num_proofs, _p(ni_), max_num_inputs,
             num_witness_secs, _p(a), *[ctypes.byref(h) for h in hs])
    out = []
    for h in hs:
        t = Pqx.__new__(Pqx)
        t.ctx, t._h, t.P = ctx, h, P
        dims = np.zeros(4, dtype=np.uint64)
        npf = np.zeros(P, dtype=np.uint64)
        nin = np.zeros(P, dtype=np.uint64)
        assert lib().spg_pqx_shape(h, _p(dims), _p(npf), _p(nin)) == 0
        t.n = int(sum(int(x) * int(y) for x, y in zip(npf, nin)))
        out.append(t)
    return tuple(out)


def _abc_args(inst, num_instances, num_witness_secs, max_num_inputs, num_inputs, evals_rx):
    """the shared arguments of the eval-table entries (after the context), the output tables' instance count and
    their scalars"""
    Pm = inst.num_instances
    assert len(num_inputs) >= max(Pm, 1), "num_inputs: one entry per instance"
    ni_ = np.asarray(num_inputs, dtype=np.uint64)
    n = sum(int(num_witness_secs) * int(x) for x in num_inputs[:Pm])
    return ni_, Pm, n, (inst.handle, num_instances, num_witness_secs, max_num_inputs, _p(ni_), evals_rx.handle)


def r1cs_eval_tables(ctx, inst, num_instances, num_witness_secs, max_num_inputs, num_inputs, evals_rx):
    """R1CSInstance::compute_eval_table_sparse_disjoint_rounds (src/r1csinstance.rs:484-534) on evals_rx (a Buf, eq(rx)):
    (A, B, C) as resident Pqx tables of the handle's own matrix count (1 for a shared instance), one proof row, x in
    natural order"""
    keep, Pm, n, args = _abc_args(inst, num_instances, num_witness_secs, max_num_inputs, num_inputs, evals_rx)
    hs = [ctypes.c_void_p() for _ in range(3)]
    ctx.call("spg_r1cs_eval_tables", *args, *[ctypes.byref(h) for h in hs])
    return tuple(_pqx_from_handle(ctx, h, Pm, n) for h in hs)


def r1cs_abc_poly(ctx, inst, num_instances, num_witness_secs, max_num_inputs, num_inputs, evals_rx, rA, rB, rC):
    """prove_abc_gen (src/r1csproof.rs:430-465): r_A A + r_B B + r_C C of r1cs_eval_tables in new_rev order, one Pqx"""
    keep, Pm, n, args = _abc_args(inst, num_instances, num_witness_secs, max_num_inputs, num_inputs, evals_rx)
    h = ctypes.c_void_p()
    ctx.call("spg_r1cs_abc_poly", *args, _p(_scalars(rA)), _p(_scalars(rB)), _p(_scalars(rC)), ctypes.byref(h))
    return _pqx_from_handle(ctx, h, Pm, n)


def zk_proof_len(num_rounds):
    """bytes of bincode(ZKSumcheckInstanceProof) with num_rounds cubic rounds"""
    return 24 + 328 * num_rounds


def _zk_prove(ctx, what, head, tail, rounds, n_claims, cap):
    n = ctypes.c_size_t(0)
    cap = zk_proof_len(rounds) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    r = np.zeros((max(rounds, 1), 4), dtype=np.uint64)
    claims = np.zeros((n_claims, 4), dtype=np.uint64)
    blind = np.zeros(4, dtype=np.uint64)
    rc = getattr(lib(), what)(ctx.handle, *head, *tail, _p(out), cap, ctypes.byref(n), _p(r), _p(claims), _p(blind))
    ctx.last_len = int(n.value)
    ctx.check(rc, what)
    return out[:n.value].tobytes(), r[:rounds], claims, blind


def zk_phase1_prove(ctx, gens, nx, nq, np_, Ap, Aq, Ax, B, C, D, transcript, tape, claim=None, blind_claim=None,
                    cap=None):
    """ZKSumcheckInstanceProof::prove_cubic_with_additive_term_disjoint_rounds (src/sumcheck.rs:1067-1380) with comb
    A (B C - D): Ap, Aq, Ax (Bufs) and B, C, D (Pqx) are bound in place. Returns (proof bytes, r [rounds, 4],
    claims [4, 4] = (Ap Aq Ax, B, C, D), blinds_evals[last]); ctx.last_len keeps *len."""
    c, b = _opt(claim), _opt(blind_claim)
    head = (gens.handle, _optp(c), _optp(b), nx, nq, np_)
    tail = (Ap.handle, Aq.handle, Ax.handle, B._h, C._h, D._h, transcript.handle, tape.handle)
    res = _zk_prove(ctx, "spg_zk_phase1_prove", head, tail, nx + nq + np_, 4, cap)
    Ap.n, Aq.n, Ax.n = 1, 1, 1
    return res


def zk_phase2_prove(ctx, gens, ny, nw, np_, single_inst, num_witness_secs, eq, ABC, Z, transcript, tape, claim=None,
                    blind_claim=None, cap=None):
    """ZKSumcheckInstanceProof::prove_cubic_disjoint_rounds (src/sumcheck.rs:788-1065) with comb A B C: eq (a Buf),
    ABC and Z (Pqx, q bound) are bound in place. Returns (proof bytes, r, claims [3, 4] = (eq, ABC, Z),
    blinds_evals[last])."""
    c, b = _opt(claim), _opt(blind_claim)
    head = (gens.handle, _optp(c), _optp(b), ny, nw, np_, 1 if single_inst else 0, num_witness_secs)
    tail = (eq.handle, ABC._h, Z._h, transcript.handle, tape.handle)
    res = _zk_prove(ctx, "spg_zk_phase2_prove", head, tail, ny + nw + np_, 3, cap)
    eq.n = 1
    return res


def zk_sumcheck_verify(ctx, gens, comm_claim, num_rounds, transcript, proof, degree_bound=3):
    """ZKSumcheckInstanceProof::verify (src/sumcheck.rs:94-189): (accepted, comm_claim_post [32 bytes], r
    [num_rounds, 4], the failed check's name)"""
    cc = np.frombuffer(bytes(comm_claim), dtype=np.uint8).copy()
    assert cc.shape[0] == 32, "comm_claim: a 32-byte compressed point"
    pb = _bytes_arr(proof)
    post = np.zeros(32, dtype=np.uint8)
    r = np.zeros((max(num_rounds, 1), 4), dtype=np.uint64)
    rc = lib().spg_zk_sumcheck_verify(ctx.handle, gens.handle, _p(cc), num_rounds, degree_bound, transcript.handle,
                                      _p(pb), len(proof), _p(post), _p(r))
    ok, why = _verify_result(ctx, rc, "spg_zk_sumcheck_verify")
    return ok, post.tobytes(), r[:num_rounds], why


# ---- memory checking and the grand-product argument on device vectors (csrc/prodc.hip)
def _buf_from_handle(ctx, h):
    b = Buf.__new__(Buf)
    b.ctx = ctx
    b._h = h
    b.n = int(lib().spg_buf_len(h))
    return b


def _buf_array(bufs):
    """a C array of spg_buf* (kept alive by the caller for the call's duration)"""
    return (ctypes.c_void_p * max(len(bufs), 1))(*[b.handle.value for b in bufs])


def _sync_len(bufs):
    for b in bufs:
        b.n = int(lib().spg_buf_len(b.handle))


def hash_layer(ctx, eval_table, addrs, derefs, read_ts, audit_ts, r_hash, r_multiset):
    """Layers::build_hash_layer (src/sparse_mlpoly.rs:612-687) on Bufs: eval_table, audit_ts of num_mem_cells scalars;
    addrs, derefs, read_ts lists of n Bufs of num_ops scalars. Returns (init, reads, writes, audit): new Bufs (reads,
    writes lists of n)."""
    n = len(addrs)
    if n == 0 or len(derefs) != n or len(read_ts) != n:
        raise ValueError("hash_layer: addrs, derefs, read_ts must be n >= 1 vectors each")
    if audit_ts.n != eval_table.n:
        raise ValueError("hash_layer: audit_ts must hold one scalar per memory cell")
    if any(b.n != addrs[0].n for b in list(addrs) + list(derefs) + list(read_ts)):
        raise ValueError("hash_layer: addrs, derefs, read_ts must have one length")
    a, d, t = _buf_array(addrs), _buf_array(derefs), _buf_array(read_ts)
    init, audit = ctypes.c_void_p(), ctypes.c_void_p()
    reads, writes = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    ctx.call("spg_hash_layer", eval_table.handle, a, d, t, n, audit_ts.handle, _p(_scalars(r_hash)),
             _p(_scalars(r_multiset)), ctypes.byref(init), reads, writes, ctypes.byref(audit))
    mk = lambda h: _buf_from_handle(ctx, ctypes.c_void_p(h))  # noqa: E731
    return mk(init.value), [mk(h) for h in reads], [mk(h) for h in writes], mk(audit.value)


class ProductCircuits(_Handle):
    """nc ProductCircuits of M leaves each (src/product_tree.rs:18-108) built on the device from Bufs of one
    power-of-two length M >= 2 (spg_prodc_*); the inputs are left unchanged."""

    _free = "spg_prodc_free"

    def __init__(self, ctx, polys):
        polys = list(polys)
        if not polys or any(b.n != polys[0].n for b in polys):
            raise ValueError("ProductCircuits: one or more polynomials of one length")
        M = polys[0].n
        if M < 2 or M & (M - 1):
            raise ValueError("ProductCircuits: the length must be a power of two >= 2")
        self.ctx = ctx
        self.nc, self.M = len(polys), M
        self._h = ctypes.c_void_p()
        ctx.call("spg_prodc_new", _buf_array(polys), self.nc, ctypes.byref(self._h))

    @property
    def shape(self):
        """(nc, num_leaves) as the library holds them"""
        nc, m = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib().spg_prodc_shape(self._h, ctypes.byref(nc), ctypes.byref(m)) == 0
        return int(nc.value), int(m.value)

    def evaluate(self):
        """ProductCircuit::evaluate of every circuit: [nc, 4]"""
        out = np.zeros((self.nc, 4), dtype=np.uint64)
        self.ctx.call("spg_prodc_evaluate", self._h, _p(out))
        return out

    def layer(self, c, k):
        """(left_vec[k], right_vec[k]) of circuit c: M >> (k + 1) scalars each"""
        if not (0 <= c < self.nc) or not (0 <= k < self.M.bit_length() - 1):
            raise ValueError("ProductCircuits.layer: no such circuit layer")
        half = self.M >> (k + 1)
        left, right = np.zeros((half, 4), dtype=np.uint64), np.zeros((half, 4), dtype=np.uint64)
        self.ctx.call("spg_prodc_layer", self._h, c, k, _p(left), _p(right))
        return left, right

    def proof_size(self, nd):
        """bytes of bincode(ProductCircuitEvalProofBatched) for these circuits and nd dot-product circuits"""
        L = self.M.bit_length() - 1
        return 8 + 3 * (8 + 32 * nd) + sum(8 + j * 104 + 2 * (8 + 32 * self.nc) for j in range(L))

    def prove_batched(self, dotp, transcript, cap=None):
        """ProductCircuitEvalProofBatched::prove (src/product_tree.rs:260-396): dotp a list of (left, right, weight)
        Bufs of M/2 scalars, bound in place. Returns (proof bytes, rand [log2 M, 4]); the circuits are consumed."""
        flat = [b for tr in dotp for b in tr]
        if any(len(tr) != 3 for tr in dotp) or any(b.n != self.M // 2 for b in flat):
            raise ValueError("prove_batched: dot-product circuits are (left, right, weight) of M/2 scalars each")
        cap = self.proof_size(len(dotp)) if cap is None else cap
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n, rl = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rand = np.zeros((self.M.bit_length(), 4), dtype=np.uint64)
        rc = lib().spg_prodc_prove_batched(self.ctx.handle, self._h, _buf_array(flat), len(dotp), transcript.handle,
                                           _p(out), cap, ctypes.byref(n), _p(rand), ctypes.byref(rl))
        self.last_len = int(n.value)
        self.ctx.check(rc, "spg_prodc_prove_batched")
        _sync_len(flat)
        return out[:n.value].tobytes(), rand[:rl.value].copy()


def prove_cubic_batched(ctx, claim, num_rounds, A_par, B_par, C_par, A_seq, B_seq, C_seq, coeffs, transcript):
    """SumcheckInstanceProof::prove_cubic_batched with comb A B C (src/sumcheck.rs:264-434): pairs (A_par[i], B_par[i])
    sharing C_par (None allowed without pairs), triples (A_seq[i], B_seq[i], C_seq[i]); every Buf of one length 2^k,
    k >= num_rounds, bound in place. Returns (polys [num_rounds, 3, 4], r [num_rounds, 4], claims_par [2 n_par + 1, 4]
    (A finals, B finals, C_par[0]; empty without C_par), claims_seq [3, n_seq, 4])."""
    A_par, B_par, A_seq, B_seq, C_seq = (list(x) for x in (A_par, B_par, A_seq, B_seq, C_seq))
    n_par, n_seq = len(A_par), len(A_seq)
    if len(B_par) != n_par or len(B_seq) != n_seq or len(C_seq) != n_seq or n_par + n_seq == 0:
        raise ValueError("prove_cubic_batched: one B per A (and one C per sequential A), at least one term")
    if n_par and C_par is None:
        raise ValueError("prove_cubic_batched: the pairs need C_par")
    bufs = A_par + B_par + ([C_par] if C_par is not None else []) + A_seq + B_seq + C_seq
    n = bufs[0].n
    if n == 0 or n & (n - 1) or any(b.n != n for b in bufs) or (1 << num_rounds) > n:
        raise ValueError("prove_cubic_batched: every vector must hold 2^k scalars, one k >= num_rounds")
    co = _scalars(coeffs)
    if co.shape[0] != n_par + n_seq:
        raise ValueError("prove_cubic_batched: one coefficient per term")
    polys = np.zeros((max(num_rounds, 1), 3, 4), dtype=np.uint64)
    r = np.zeros((max(num_rounds, 1), 4), dtype=np.uint64)
    cpar = np.zeros((2 * n_par + 1, 4), dtype=np.uint64)
    cseq = np.zeros((3, max(n_seq, 1), 4), dtype=np.uint64)
    ctx.call("spg_prove_cubic_batched", _p(_scalars(claim)), num_rounds, _buf_array(A_par), _buf_array(B_par), n_par,
             C_par.handle if C_par is not None else None, _buf_array(A_seq), _buf_array(B_seq), _buf_array(C_seq), n_seq,
             _p(co), transcript.handle, _p(polys), _p(r), _p(cpar), _p(cseq))
    _sync_len(bufs)
    return polys[:num_rounds], r[:num_rounds], cpar if C_par is not None else cpar[:0], cseq[:, :n_seq]


def r1cs_multi_evaluate(ctx, inst, num_instances, rx, ry):
    """R1CSInstance::multi_evaluate -> (3 * num_instances, 4) limbs [A_0, B_0, C_0, A_1, ...]"""
    rx = _scalars(rx)
    ry = _scalars(ry)
    out = np.zeros((3 * num_instances, 4), dtype=np.uint64)
    ctx.call("spg_r1cs_multi_evaluate", inst.handle, _p(rx), rx.shape[0], _p(ry), ry.shape[0], _p(out))
    return out


class R1CSWitness(_Handle):
    """Witness sections (Vec<&ProverWitnessSecInfo>) resident in HBM. `secs` is workload.CViews().secs.
    shard=(p0, p1): upload only instances [p0, p1) of the per-instance sections (sharded proving)."""

    _free = "spg_r1cs_witness_free"

    def __init__(self, ctx, secs, nws, shard=None):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        if shard is None:
            ctx.call("spg_r1cs_witness_new", secs, nws, ctypes.byref(self._h))
        else:
            ctx.call("spg_r1cs_witness_new_shard", secs, nws, shard[0], shard[1], ctypes.byref(self._h))


def r1cs_prove(ctx, gens, inst, witness, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs,
               transcript, tape, cap=1 << 22):
    """R1CSProof::prove -> (bincode bytes, [rp, rq_rev, rx, rw||ry] as (k, 4) uint64 arrays)."""
    buf = ctx.out_buf(cap)
    ln = ctypes.c_size_t(0)
    ch = np.zeros((4096, 4), dtype=np.uint64)
    chl = (ctypes.c_size_t * 4)()
    npf = (ctypes.c_size_t * num_instances)(*num_proofs)
    nin = (ctypes.c_size_t * num_instances)(*num_inputs)
    ctx.call("spg_r1cs_prove", gens.handle, inst.handle, num_instances, max_num_proofs, npf, max_num_inputs, nin,
             witness.handle, transcript.handle, tape.handle, _p(buf), cap, ctypes.byref(ln), _p(ch), chl)
    out, o = [], 0
    for L in list(chl):
        out.append(ch[o:o + L].copy())
        o += L
    return buf[: ln.value].tobytes(), out


# ---- witness satisfiability (spg_pqx_sat_check, spg_r1cs_sat_check, spg_snark_check, spg_set_check_sat) ----
class CSatReport(ctypes.Structure):  # spg_sat_report
    _fields_ = [("rows", ctypes.c_uint64), ("violations", ctypes.c_uint64), ("p", ctypes.c_uint64),
                ("q", ctypes.c_uint64), ("row", ctypes.c_uint64), ("az", ctypes.c_uint64 * 4),
                ("bz", ctypes.c_uint64 * 4), ("cz", ctypes.c_uint64 * 4)]


class CSnarkReport(ctypes.Structure):  # spg_snark_report
    _fields_ = [("sat", CSatReport * 3), ("component", ctypes.c_uint64 * 3), ("perm_products", ctypes.c_uint64 * 3),
                ("io_point", ctypes.c_int64), ("first", ctypes.c_int64)]


# spg_snark_report: the stages (indices of sat / component), the values of `first`, and the component numbers
SAT_BLOCK, SAT_PAIRWISE, SAT_PERM_ROOT = 0, 1, 2
FIRST_NONE, FIRST_PERM_EXEC, FIRST_PERM_PHY, FIRST_PERM_VIR, FIRST_IO = -1, 3, 4, 5, 6
PERM_EXEC, PERM_PHY, PERM_VIR = 0, 1, 2  # perm_products
PAIRWISE_CONSIS, PAIRWISE_PHY, PAIRWISE_VIR = 0, 1, 2
PERM_ROOT_EXEC, PERM_ROOT_INIT_PHY, PERM_ROOT_INIT_VIR, PERM_ROOT_PHY, PERM_ROOT_VIR = 0, 1, 2, 3, 4
SAT_STAGES = ("block", "pairwise", "perm_root")

_Q = (1 << 252) + 27742317777372353535851937790883648493
_RINV = pow(1 << 256, -1, _Q)

SatReport = collections.namedtuple("SatReport", "rows violations p q row az bz cz")
SnarkReport = collections.namedtuple("SnarkReport", "sat component perm_products io_point first")


def _sat_report(c):
    """spg_sat_report with Python integers; az, bz, cz out of Montgomery form (None when nothing is violated)"""
    val = lambda limbs: sum(int(limbs[i]) << (64 * i) for i in range(4)) * _RINV % _Q
    if not c.violations:
        return SatReport(int(c.rows), 0, None, None, None, None, None, None)
    return SatReport(int(c.rows), int(c.violations), int(c.p), int(c.q), int(c.row), val(c.az), val(c.bz), val(c.cz))


def pqx_sat_check(ctx, Az, Bz, Cz):
    """spg_pqx_sat_check: Az[i] * Bz[i] == Cz[i] over three tables as r1cs_multiply_vec_block returns them"""
    rep = CSatReport()
    ctx.call("spg_pqx_sat_check", Az.handle, Bz.handle, Cz.handle, ctypes.byref(rep))
    return _sat_report(rep)


def r1cs_sat_check(ctx, inst, witness, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs):
    """spg_r1cs_sat_check (R1CSInstance::is_sat over every execution of every instance): the shape and witness
    arguments of r1cs_prove; a collective under set_comm"""
    rep = CSatReport()
    npf = (ctypes.c_size_t * num_instances)(*num_proofs)
    nin = (ctypes.c_size_t * num_instances)(*num_inputs)
    ctx.call("spg_r1cs_sat_check", inst.handle, num_instances, max_num_proofs, npf, max_num_inputs, nin,
             witness.handle, ctypes.byref(rep))
    return _sat_report(rep)


def snark_check(ctx, block, pairwise, perm_root, witness, vars_gens, transcript):
    """spg_snark_check: everything a verifier would reject a bad witness for, without proving. `transcript` is a
    throwaway in the state a prove would start from. -> (SnarkReport, spg_last_error's text for the first failure)"""
    rep = CSnarkReport()
    ctx.call("spg_snark_check", block.handle, pairwise.handle, perm_root.handle, witness.handle, vars_gens.handle,
             transcript.handle, ctypes.byref(rep))
    out = SnarkReport(tuple(_sat_report(r) for r in rep.sat), tuple(int(x) for x in rep.component),
                      tuple(int(x) for x in rep.perm_products), int(rep.io_point), int(rep.first))
    return out, (lib().spg_last_error(ctx.handle).decode() if out.first >= 0 else "")


class CWitnessComm(ctypes.Structure):
    _fields_ = [("num_instances", ctypes.c_size_t), ("num_proofs", ctypes.POINTER(ctypes.c_size_t)),
                ("num_inputs", ctypes.POINTER(ctypes.c_size_t)), ("comm_len", ctypes.POINTER(ctypes.c_size_t)),
                ("comms", ctypes.c_void_p)]


def r1cs_gens_commit(ctx, gens, Z):
    """DensePolynomial::commit (no blinds) with gens.gens_pc -> list of 32-byte Hyrax row commitments"""
    z = _scalars(Z)
    out = np.zeros(32 * 4096, dtype=np.uint8)
    L = ctypes.c_size_t(0)
    ctx.call("spg_r1cs_gens_commit", gens.handle, _p(z), z.shape[0], _p(out), out.shape[0], ctypes.byref(L))
    return [out[32 * i: 32 * i + 32].tobytes() for i in range(L.value)]


def r1cs_verify(ctx, gens, num_instances, max_num_proofs, num_proofs, max_num_inputs, sections, num_cons, evals,
                transcript, proof):
    """R1CSProof::verify (src/r1csproof.rs:687-954). sections: per witness section (num_proofs, num_inputs, comms)
    with one entry per instance (comms: lists of 32-byte row commitments). Returns (ok, reason, challenges)."""
    keep = []
    secs = (CWitnessComm * len(sections))()
    for i, (npf, nin, comms) in enumerate(sections):
        a, b = (ctypes.c_size_t * len(npf))(*npf), (ctypes.c_size_t * len(nin))(*nin)
        cl = (ctypes.c_size_t * len(comms))(*[len(c) for c in comms])
        blob = np.frombuffer(b"".join(b"".join(c) for c in comms) or b"\0", dtype=np.uint8).copy()
        keep += [a, b, cl, blob]
        secs[i] = CWitnessComm(len(npf), a, b, cl, blob.ctypes.data)
    ev = _scalars(evals)
    buf = _bytes_arr(proof)
    ch = np.zeros((4096, 4), dtype=np.uint64)
    chl = (ctypes.c_size_t * 4)()
    npf = (ctypes.c_size_t * num_instances)(*num_proofs)
    rc = lib().spg_r1cs_verify(ctx.handle, gens.handle, num_instances, max_num_proofs, npf, max_num_inputs, secs,
                               len(sections), num_cons, _p(ev), transcript.handle, _p(buf), len(proof), _p(ch), chl)
    ok, why = _verify_result(ctx, rc, "spg_r1cs_verify")
    if not ok:
        return False, why, None
    out, o = [], 0
    for L in list(chl):
        out.append(ch[o:o + L].copy())
        o += L
    return True, "", out


def shard_range(num_instances, rank, nranks):
    """instances [p0, p1) held by `rank` in a sharded R1CSProof (include/spg.h, spg_set_comm): balanced split,
    the first num_instances % nranks ranks hold one instance more (same rule as r1cs.hip Prover::shard_begin)"""
    def begin(r):
        return r * (num_instances // nranks) + min(r, num_instances % nranks)
    return begin(rank), begin(rank + 1)


class SparkCommitment(_Handle):
    """SparseMatPolynomial::multi_commit over the 3P matrices of an R1CS instance (src/sparse_mlpoly.rs:566-587)
    with SparseMatPolyCommitmentGens::new(label, nvx, nvy, gens_nnz, gens_batch). The dense representation
    stays in HBM for SparkCommitment.prove. `cinst` is a workload.CViews().inst."""

    _free = "spg_spark_free"

    def __init__(self, ctx, cinst, label, gens_nnz, gens_batch=3, cap=1 << 22):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        if isinstance(label, str):
            label = label.encode()
        buf = np.zeros(cap, dtype=np.uint8)
        ln = ctypes.c_size_t(0)
        lb = (ctypes.c_uint8 * len(label)).from_buffer_copy(label)
        ctx.call("spg_spark_commit", ctypes.byref(cinst), lb, len(label), gens_nnz, gens_batch, ctypes.byref(self._h),
                 _p(buf), cap, ctypes.byref(ln))
        self.bytes = buf[: ln.value].tobytes()

    def prove(self, rx, ry, evals, transcript, tape, cap=1 << 24):
        """SparseMatPolyEvalProof::prove (src/sparse_mlpoly.rs:1497-1564) -> bincode bytes"""
        rx = _scalars(rx)
        ry = _scalars(ry)
        ev = _scalars(evals)
        buf = self.ctx.out_buf(cap)
        ln = ctypes.c_size_t(0)
        self.ctx.call("spg_spark_prove", self._h, _p(rx), rx.shape[0], _p(ry), ry.shape[0], _p(ev), ev.shape[0],
                      transcript.handle, tape.handle, _p(buf), cap, ctypes.byref(ln))
        return buf[: ln.value].tobytes()

    def verify(self, rx, ry, evals, transcript, proof):
        """SparseMatPolyEvalProof::verify (src/sparse_mlpoly.rs:1566-1610) -> (ok, reason)"""
        rx, ry, ev = _scalars(rx), _scalars(ry), _scalars(evals)
        buf = _bytes_arr(proof)
        rc = lib().spg_spark_verify(self.ctx.handle, self._h, _p(rx), rx.shape[0], _p(ry), ry.shape[0], _p(ev),
                                    ev.shape[0], transcript.handle, _p(buf), len(proof))
        return _verify_result(self.ctx, rc, "spg_spark_verify")


class SnarkComp(_Handle):
    """SNARK::multi_encode (multi=True) / SNARK::encode of one R1CS instance (src/lib.rs:793-829); `cinst` is a
    workload.SnarkViews().block / .pairwise / .perm_root (spg_snark_instance)."""

    _free = "spg_snark_comp_free"

    def __init__(self, ctx, cinst, multi=False):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        ctx.call("spg_snark_encode", ctypes.byref(cinst), 1 if multi else 0, ctypes.byref(self._h))

    def comm_bytes(self, as_list):
        """bincode(Vec<ComputationCommitment>) (as_list) or bincode(ComputationCommitment) (spg_snark_comm_bytes)"""
        ln = ctypes.c_size_t(0)
        lib().spg_snark_comm_bytes(self.ctx.handle, self._h, 1 if as_list else 0, None, 0, ctypes.byref(ln))
        buf = np.zeros(max(ln.value, 1), dtype=np.uint8)
        self.ctx.call("spg_snark_comm_bytes", self._h, 1 if as_list else 0, _p(buf), ln.value, ctypes.byref(ln))
        return buf[: ln.value].tobytes()

    def comm_map(self):
        """block_comm_map: one list of matrix indices 3p + m per commitment (spg_snark_comm_map)"""
        idx = np.zeros(1 << 16, dtype=np.uintp)
        lens = np.zeros(1 << 12, dtype=np.uintp)
        n = ctypes.c_size_t(0)
        self.ctx.call("spg_snark_comm_map", self._h, _p(idx), len(idx), _p(lens), len(lens), ctypes.byref(n))
        out, o = [], 0
        for g in range(n.value):
            out.append([int(x) for x in idx[o:o + int(lens[g])]])
            o += int(lens[g])
        return out

    @classmethod
    def load(cls, ctx, comm, as_list, comm_map, num_cons, gens):
        """a verifier-side instance from ComputationCommitment bytes (spg_snark_comm_load): comm_map = block_comm_map
        for a list, num_cons = block_num_cons / pairwise_check_num_cons / perm_root_num_cons, gens = the
        SNARKGens::new(num_cons, num_vars, num_instances, num_nz_entries) arguments"""
        c = cls.__new__(cls)
        c.ctx = ctx
        c._h = ctypes.c_void_p()
        buf = _bytes_arr(comm)
        flat = np.array([k for l in (comm_map or []) for k in l] or [0], dtype=np.uintp)
        lens = np.array([len(l) for l in (comm_map or [])] or [0], dtype=np.uintp)
        ctx.call("spg_snark_comm_load", _p(buf), len(comm), 1 if as_list else 0, _p(flat), _p(lens),
                 len(comm_map or []), num_cons, *gens, ctypes.byref(c._h))
        return c


class SnarkWitness(_Handle):
    """SNARK::prove's run-time inputs with block_vars / exec inputs resident in HBM (workload.SnarkViews().inputs)"""

    _free = "spg_snark_witness_free"

    def __init__(self, ctx, cinputs):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        ctx.call("spg_snark_witness_new", ctypes.byref(cinputs), ctypes.byref(self._h))


def snark_prove(ctx, block, pairwise, perm_root, witness, vars_gens, transcript, tape, cap=1 << 24):
    """SNARK::prove (src/lib.rs:971-2746) -> bincode(SNARK)"""
    buf = ctx.out_buf(cap)
    ln = ctypes.c_size_t(0)
    ctx.call("spg_snark_prove", block.handle, pairwise.handle, perm_root.handle, witness.handle, vars_gens.handle,
             transcript.handle, tape.handle, _p(buf), cap, ctypes.byref(ln))
    return buf[: ln.value].tobytes()


def snark_verify(ctx, block, pairwise, perm_root, inputs, vars_gens, transcript, proof):
    """SNARK::verify (src/lib.rs:2750-3881) of bincode(SNARK) bytes against the encoded instances and the public
    inputs (`inputs`: workload.SnarkViews().inputs; only its sizes, input / output and init memory lists are read).
    Returns (True, "") when the proof verifies, (False, reason) when it does not; raises on bad arguments."""
    buf = _bytes_arr(proof)
    rc = lib().spg_snark_verify(ctx.handle, block.handle, pairwise.handle, perm_root.handle, ctypes.byref(inputs),
                                vars_gens.handle, transcript.handle, _p(buf), len(proof))
    return _verify_result(ctx, rc, "spg_snark_verify")


def snark_verify_public(ctx, block, pairwise, perm_root, public, vars_gens, transcript, proof):
    """SNARK::verify from what the reference verifier is given (spg_snark_verify_public): SnarkComp.load'ed
    commitments and `public` (a workload.CSnarkPublic). Returns (True, "") / (False, reason); raises on bad arguments."""
    buf = _bytes_arr(proof)
    rc = lib().spg_snark_verify_public(ctx.handle, block.handle, pairwise.handle, perm_root.handle,
                                       ctypes.byref(public), vars_gens.handle, transcript.handle, _p(buf), len(proof))
    return _verify_result(ctx, rc, "spg_snark_verify_public")


def points_sum_compress(parts):
    """spg_points_sum_compress (host only): encoding of the sum of 128-byte partial points"""
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8).copy() if parts else np.zeros(1, np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    rc = lib().spg_points_sum_compress(_p(buf), len(parts), _p(out))
    assert rc == 0, rc
    return out.tobytes()


# ---- Hyrax dense polynomial commitments and evaluation proofs on device vectors (csrc/polyeval.hip)
class PolyGens(_Handle):
    """PolyCommitmentGens::new(num_vars, label) (src/dense_mlpoly.rs:31-38), resident in HBM: n = 2^(num_vars -
    num_vars/2) row generators G_0 .. G_{n-1}, G_n for evaluations, and h."""

    _free = "spg_poly_gens_free"

    def __init__(self, ctx, label, num_vars):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        lb = np.frombuffer(bytes(label), dtype=np.uint8).copy()
        ctx.call("spg_poly_gens_new", _p(lb), len(label), num_vars, ctypes.byref(self._h))
        self.n = int(lib().spg_poly_gens_n(self._h))

    def compressed(self):
        """[n + 2, 32]: G_0 .. G_n, h"""
        out = np.zeros((self.n + 2, 32), dtype=np.uint8)
        self.ctx.call("spg_poly_gens_download", self._h, _p(out))
        return out


def _opt(x):
    return None if x is None else _scalars(x)


def _optp(a):
    return None if a is None else _p(a)


def _bytes_arr(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(1, np.uint8)


def _prove_call(ctx, what, call, cap):
    """the provers' output convention: with cap None the size is asked for first (a call whose output does not fit
    sets *len, returns SPG_E_ARG and touches neither transcript nor tape). ctx.last_len keeps *len of the last call."""
    n = ctypes.c_size_t(0)
    if cap is None:
        probe = np.zeros(1, dtype=np.uint8)
        rc = call(_p(probe), 0, ctypes.byref(n))
        ctx.last_len = int(n.value)
        if rc != SPG_E_ARG or n.value == 0:
            ctx.check(rc, what)
            raise SpgError(f"{what}: no proof size")
        cap = int(n.value)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    rc = call(_p(out), cap, ctypes.byref(n))
    ctx.last_len = int(n.value)
    ctx.check(rc, what)
    return out[:n.value].tobytes()


def _verify_result(ctx, rc, what):
    if rc == SPG_E_VERIFY:
        return False, lib().spg_last_error(ctx.handle).decode(errors="replace")
    ctx.check(rc, what)
    return True, ""


def poly_commit(ctx, gens, Z, num_vars, offset=0, blinds=None):
    """DensePolynomial::commit / commit_with_blind (src/dense_mlpoly.rs:184-256) of Z[offset : offset + 2^num_vars] (a
    Buf): [L, 32] row commitments, L = 2^(num_vars/2); blinds: L scalars or None (zeros)."""
    rows = 1 << (max(int(num_vars), 0) // 2)
    out = np.zeros((rows, 32), dtype=np.uint8)
    b = _opt(blinds)
    L = ctypes.c_size_t(0)
    ctx.call("spg_poly_commit", gens.handle, Z.handle, offset, num_vars, _optp(b), _p(out), out.size, ctypes.byref(L))
    return out[:L.value]


def poly_eval_prove(ctx, gens, Z, r, Zr, transcript, tape, offset=0, blinds=None, blind_Zr=None, cap=None):
    """PolyEvalProof::prove (src/dense_mlpoly.rs:437-490) of Z[offset : offset + 2^len(r)] at r with the claimed value
    Zr. Returns (bincode(PolyEvalProof), C_Zr_prime)."""
    rr, zr, b, bz = _scalars(r), _scalars(Zr), _opt(blinds), _opt(blind_Zr)
    czr = np.zeros(32, dtype=np.uint8)

    def call(out, c, n):
        return lib().spg_poly_eval_prove(ctx.handle, gens.handle, Z.handle, offset, _p(rr), rr.shape[0], _p(zr),
                                         _optp(b), _optp(bz), transcript.handle, tape.handle, out, c, n, _p(czr))

    proof = _prove_call(ctx, "spg_poly_eval_prove", call, cap)
    return proof, czr.tobytes()


def poly_eval_verify(ctx, gens, r, C_Zr, comm, transcript, proof):
    """PolyEvalProof::verify (src/dense_mlpoly.rs:492-514): comm [L, 32], C_Zr 32 bytes. Returns (ok, reason)."""
    rr, cz, cm, pf = _scalars(r), _bytes_arr(C_Zr), np.ascontiguousarray(comm, dtype=np.uint8), _bytes_arr(proof)
    rc = lib().spg_poly_eval_verify(ctx.handle, gens.handle, _p(rr), rr.shape[0], _p(cz), _p(cm), cm.size // 32,
                                    transcript.handle, _p(pf), len(proof))
    return _verify_result(ctx, rc, "spg_poly_eval_verify")


def poly_eval_verify_plain(ctx, gens, r, Zr, comm, transcript, proof):
    """PolyEvalProof::verify_plain (src/dense_mlpoly.rs:516-528). Returns (ok, reason)."""
    rr, zr, cm, pf = _scalars(r), _scalars(Zr), np.ascontiguousarray(comm, dtype=np.uint8), _bytes_arr(proof)
    rc = lib().spg_poly_eval_verify_plain(ctx.handle, gens.handle, _p(rr), rr.shape[0], _p(zr), _p(cm), cm.size // 32,
                                          transcript.handle, _p(pf), len(proof))
    return _verify_result(ctx, rc, "spg_poly_eval_verify_plain")


def poly_eval_prove_batched_points(ctx, gens, Z, num_vars, r_list, Zr_list, transcript, tape, offset=0, cap=None):
    """PolyEvalProof::prove_batched_points (src/dense_mlpoly.rs:531-622): r_list [K, num_vars, 4], Zr_list [K, 4] on
    the polynomial Z[offset : offset + 2^num_vars]. Returns bincode(Vec<PolyEvalProof>)."""
    zr = _scalars(Zr_list)
    K = zr.shape[0]
    rl = np.ascontiguousarray(r_list, dtype=np.uint64).reshape(K * num_vars, 4) if K * num_vars else np.zeros((1, 4), np.uint64)

    def call(out, c, n):
        return lib().spg_poly_eval_prove_batched_points(ctx.handle, gens.handle, Z.handle, offset, num_vars, _p(rl), K,
                                                        _p(zr), transcript.handle, tape.handle, out, c, n)

    return _prove_call(ctx, "spg_poly_eval_prove_batched_points", call, cap)


def poly_eval_verify_plain_batched_points(ctx, gens, num_vars, r_list, Zr_list, comm, transcript, proof):
    """PolyEvalProof::verify_plain_batched_points (src/dense_mlpoly.rs:624-685). Returns (ok, reason)."""
    zr = _scalars(Zr_list)
    K = zr.shape[0]
    rl = np.ascontiguousarray(r_list, dtype=np.uint64).reshape(K * num_vars, 4) if K * num_vars else np.zeros((1, 4), np.uint64)
    cm, pf = np.ascontiguousarray(comm, dtype=np.uint8), _bytes_arr(proof)
    rc = lib().spg_poly_eval_verify_plain_batched_points(ctx.handle, gens.handle, num_vars, _p(rl), K, _p(zr), _p(cm),
                                                         cm.size // 32, transcript.handle, _p(pf), len(proof))
    return _verify_result(ctx, rc, "spg_poly_eval_verify_plain_batched_points")


def _cat_points(r_list):
    lens = [len(r) for r in r_list]
    flat = [_scalars(r) for r in r_list if len(r)]
    rl = np.ascontiguousarray(np.concatenate(flat)) if flat else np.zeros((1, 4), np.uint64)
    return rl, (ctypes.c_size_t * max(len(lens), 1))(*lens)


def poly_eval_prove_batched_instances(ctx, gens, polys, num_vars_list, r_list, Zr_list, transcript, tape, offsets=None,
                                      cap=None):
    """PolyEvalProof::prove_batched_instances (src/dense_mlpoly.rs:689-780): polynomial i is polys[i][offsets[i] :
    offsets[i] + 2^num_vars_list[i]] (Bufs; several entries may name one Buf), r_list[i] its point ([len_i, 4], fitted
    to num_vars_list[i] as the reference does), Zr_list [n, 4]. Returns bincode(Vec<PolyEvalProof>)."""
    n = len(polys)
    offs = (ctypes.c_size_t * max(n, 1))(*(offsets if offsets is not None else [0] * n))
    nvs = (ctypes.c_size_t * max(n, 1))(*num_vars_list)
    rl, lens = _cat_points(r_list)
    zr = _scalars(Zr_list)
    arr = _buf_array(polys)

    def call(out, c, ln):
        return lib().spg_poly_eval_prove_batched_instances(ctx.handle, gens.handle, arr, offs, nvs, n, _p(rl), lens,
                                                           _p(zr), transcript.handle, tape.handle, out, c, ln)

    return _prove_call(ctx, "spg_poly_eval_prove_batched_instances", call, cap)


def poly_eval_verify_plain_batched_instances(ctx, gens, r_list, Zr_list, comms, num_vars_list, transcript, proof):
    """PolyEvalProof::verify_plain_batched_instances (src/dense_mlpoly.rs:782-857): comms[i] the [L_i, 32] rows of
    polynomial i. Returns (ok, reason)."""
    n = len(comms)
    nvs = (ctypes.c_size_t * max(n, 1))(*num_vars_list)
    rl, lens = _cat_points(r_list)
    zr = _scalars(Zr_list)
    cms = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1, 32) for c in comms]
    cl = (ctypes.c_size_t * max(n, 1))(*[c.shape[0] for c in cms])
    blob = np.ascontiguousarray(np.concatenate(cms)) if n else np.zeros((1, 32), np.uint8)
    pf = _bytes_arr(proof)
    rc = lib().spg_poly_eval_verify_plain_batched_instances(ctx.handle, gens.handle, _p(rl), lens, _p(zr), _p(blob), cl,
                                                            nvs, n, transcript.handle, _p(pf), len(proof))
    return _verify_result(ctx, rc, "spg_poly_eval_verify_plain_batched_instances")


# ---- the disjoint-rounds and univariate forms of PolyEvalProof (spg_pe_*, csrc/polyeval.hip)
def _sizes(v):
    return (ctypes.c_size_t * max(len(v), 1))(*v)


def _cat_comms(C_Zr_list, comms):
    """(C_Zr blob [n, 32], rows blob, comm_lens)"""
    cz = [np.frombuffer(bytes(c), dtype=np.uint8) for c in C_Zr_list]
    cms = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1, 32) for c in comms]
    czb = np.ascontiguousarray(np.concatenate(cz)) if cz else np.zeros(32, np.uint8)
    blob = np.ascontiguousarray(np.concatenate(cms)) if cms else np.zeros((1, 32), np.uint8)
    if blob.size == 0:
        blob = np.zeros((1, 32), np.uint8)
    return czb, blob, _sizes([c.shape[0] for c in cms])


def _scalars_or_empty(x):
    return _scalars(x) if len(x) else np.zeros((1, 4), np.uint64)


def pe_prove_disjoint(ctx, gens, polys, num_proofs_list, num_inputs_list, rq, ry, Zr_list, transcript, tape,
                      offsets=None, cap=None):
    """PolyEvalProof::prove_batched_instances_disjoint_rounds (src/dense_mlpoly.rs:861-960): polynomial i is
    polys[i][offsets[i] : offsets[i] + num_proofs_list[i] * num_inputs_list[i]] (Bufs), opened at the last
    lg num_proofs entries of rq followed by ry fitted to lg num_inputs entries; Zr_list [n, 4]. Returns
    bincode(Vec<PolyEvalProof>), one proof per distinct (num_proofs, num_inputs)."""
    n = len(polys)
    offs = _sizes(offsets if offsets is not None else [0] * n)
    nps, nis = _sizes(num_proofs_list), _sizes(num_inputs_list)
    q, y, zr = _scalars_or_empty(rq), _scalars_or_empty(ry), _scalars_or_empty(Zr_list)
    arr = _buf_array(polys)

    def call(out, c, ln):
        return lib().spg_pe_prove_disjoint(ctx.handle, gens.handle, arr, offs, nps, nis, n, _p(q), len(rq), _p(y),
                                           len(ry), _p(zr), transcript.handle, tape.handle, out, c, ln)

    return _prove_call(ctx, "spg_pe_prove_disjoint", call, cap)


def pe_verify_disjoint(ctx, gens, num_proofs_list, num_inputs_list, rq, ry, C_Zr_list, comms, transcript, proof):
    """PolyEvalProof::verify_batched_instances_disjoint_rounds (src/dense_mlpoly.rs:962-1044): C_Zr_list the n
    32-byte commitments to the evaluations, comms[i] the [L_i, 32] rows of polynomial i. Returns (ok, reason)."""
    n = len(comms)
    q, y = _scalars_or_empty(rq), _scalars_or_empty(ry)
    czb, blob, cl = _cat_comms(C_Zr_list, comms)
    pf = _bytes_arr(proof)
    rc = lib().spg_pe_verify_disjoint(ctx.handle, gens.handle, _sizes(num_proofs_list), _sizes(num_inputs_list), n,
                                      _p(q), len(rq), _p(y), len(ry), _p(czb), _p(blob), cl, transcript.handle, _p(pf),
                                      len(proof))
    return _verify_result(ctx, rc, "spg_pe_verify_disjoint")


def pe_uni_evals(ctx, polys, num_vars_list, r, offsets=None):
    """the evaluations the univariate form opens (ShiftProofs::prove, src/lib.rs:417-418): [n, 4], row i =
    sum_k Z_i[k] r^k over polys[i][offsets[i] : offsets[i] + 2^num_vars_list[i]]"""
    n = len(polys)
    offs = _sizes(offsets if offsets is not None else [0] * n)
    out = np.zeros((max(n, 1), 4), dtype=np.uint64)
    rr = _scalars(r)
    ctx.call("spg_pe_uni_evals", _buf_array(polys), offs, _sizes(num_vars_list), n, _p(rr), _p(out))
    return out[:n]


def pe_prove_uni(ctx, gens, polys, num_vars_list, r, Zr_list, transcript, tape, offsets=None, cap=None):
    """PolyEvalProof::prove_uni_batched_instances (src/dense_mlpoly.rs:1046-1130): every polynomial read as univariate
    and opened at the one scalar r with the claimed values Zr_list [n, 4]. Returns (bincode(PolyEvalProof),
    C_Zr_prime)."""
    n = len(polys)
    offs = _sizes(offsets if offsets is not None else [0] * n)
    nvs = _sizes(num_vars_list)
    rr, zr = _scalars(r), _scalars_or_empty(Zr_list)
    arr = _buf_array(polys)
    czr = np.zeros(32, dtype=np.uint8)

    def call(out, c, ln):
        return lib().spg_pe_prove_uni(ctx.handle, gens.handle, arr, offs, nvs, n, _p(rr), _p(zr), transcript.handle,
                                      tape.handle, out, c, ln, _p(czr))

    proof = _prove_call(ctx, "spg_pe_prove_uni", call, cap)
    return proof, czr.tobytes()


def pe_verify_uni(ctx, gens, r, C_Zr_list, comms, poly_sizes, transcript, proof):
    """PolyEvalProof::verify_uni_batched_instances (src/dense_mlpoly.rs:1132-1203): poly_sizes as the reference takes
    them (num_vars_i = lg next_pow2(size_i)). Returns (ok, reason)."""
    n = len(comms)
    rr = _scalars(r)
    czb, blob, cl = _cat_comms(C_Zr_list, comms)
    pf = _bytes_arr(proof)
    rc = lib().spg_pe_verify_uni(ctx.handle, gens.handle, _p(rr), _p(czb), _p(blob), cl, _sizes(poly_sizes), n,
                                 transcript.handle, _p(pf), len(proof))
    return _verify_result(ctx, rc, "spg_pe_verify_uni")
