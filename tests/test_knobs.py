"""The environment table (csrc/knobs.hpp) without a GPU, through libspg_hostcheck.so's spgh_knob_table and
spgh_knob_parse: every name declared once, each kind's parse rule on its edge texts, and the project's own files
(tests, scripts, bench.py, INTEGRATION.md section 6, csrc/) checked against the table, so that a misspelled or retired
name in a form list, an undocumented switch or a getenv outside the table fails here instead of passing silently."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spartan-parallel_amd")
HC = os.environ.get("SPG_HOSTCHECK_LIB") or os.path.join(PKG, "lib", "libspg_hostcheck.so")

# (name, kind, default, re-read per call), written by hand from the read sites as they stood before the table existed
# (file of the site in the comment). Defaults as spgh_knob_table prints them: switches on / off, PRESENT and STR off /
# unset, GB in whole gigabytes, unset for a number whose site asks whether it is set (unset differs from 0 there).
PINNED = [
    # api.hip
    ("SPG_PIN", "ON", "on", 1),
    ("LOCAL_WORLD_SIZE", "INT", "0", 1),  # (also hpool.hpp)
    ("LOCAL_RANK", "INT", "0", 1),
    ("SPG_COPY_TRACE", "OFF", "off", 0),
    ("SPG_H2D", "OFF", "off", 0),
    ("SPG_H2D_THREADS", "INT", "8", 0),
    ("SPG_H2D_CHUNK_KB", "LONG", "0", 0),
    ("SPG_H2D_TRACE", "PRESENT", "off", 0),
    ("SPG_MAPPED_BUCKETS", "ON", "on", 0),
    ("SPG_FAILPOINT", "STR", "unset", 0),
    ("SPG_FAILPOINT_RANK", "INT", "0", 0),
    # hpool.hpp
    ("SPG_POOL_THREADS", "INT", "unset", 1),
    ("SPG_POOL_SPIN_US", "INT", "20000", 1),
    # hostpoly.hpp, hvec.hpp, vmsm.hpp, host.hpp
    ("SPG_TRACE", "INT", "unset", 0),
    ("SPG_TRACE_EVENTS", "PRESENT", "off", 0),
    ("SPG_AXPY_POOL", "ON", "on", 0),
    ("SPG_HOST_IFMA", "ON", "on", 0),
    ("SPG_VMSM_C", "INT", "0", 0),
    ("SPG_SLICE_MIN", "LONG", "64", 0),
    ("SPG_ENC_SPLIT", "ON", "on", 0),
    ("SPG_HOST_PREFETCH", "LONG", "3", 0),
    ("SPG_VEC_MIN", "LONG", "16", 0),
    # comb.hip
    ("SPG_COMB", "ON", "on", 0),
    ("SPG_COMB_GB", "GB", "144", 0),
    ("SPG_COMB_PAD", "ON", "on", 0),
    ("SPG_COMB_PAD_GB", "GB", "64", 0),
    ("SPG_COMB_C", "INT", "unset", 0),
    ("SPG_COMB_C_WIDE", "INT", "9", 0),
    ("SPG_COMB_C_BIG", "INT", "13", 0),
    ("SPG_COMB_WGS", "LONG", "2048", 0),
    ("SPG_COMB_GMAX", "LONG", "4", 0),
    ("SPG_COMB_GMIN", "LONG", "1", 0),
    ("SPG_BIG_COMB_G", "LONG", "2", 0),
    # msm.hip
    ("SPG_HALVED_ENC", "ON", "on", 0),  # (also hyrax.hip; snark.hip read it per prove)
    ("SPG_MSM_BIG", "ON", "on", 0),
    ("SPG_SMSM_QUAD", "ON", "on", 0),
    ("SPG_SMSM_C", "INT", "0", 1),
    ("SPG_ITEM_K", "INT", "16", 0),
    ("SPG_SEG_M", "INT", "8", 0),
    ("SPG_ROWS_CMAX", "INT", "16", 0),
    ("SPG_SEG_QUAD_MAX", "LONG", "16384", 0),
    ("SPG_FINAL_SL", "INT", "0", 0),
    ("SPG_BULLET_COMB", "ON", "on", 0),
    ("SPG_BCOMB_G", "INT", "0", 0),
    ("SPG_BCOMB_BS", "INT", "0", 0),
    ("SPG_BCOMB_R", "INT", "0", 0),
    ("SPG_BCOMB_NOTREE", "INT", "0", 0),
    # msm_big.hip, msm_var.hip
    ("SPG_BIG_COMB", "ON", "on", 0),
    ("SPG_BIG_C", "INT", "11", 0),
    ("SPG_BIG_ITEMS", "ON", "on", 0),
    ("SPG_BIG_SPT", "INT", "1", 0),
    ("SPG_BIG_PROBE", "PRESENT", "off", 0),
    ("SPG_VMSM_HOST_MAX", "LONG", "64", 0),
    ("SPG_VMSM_CH", "INT", "1024", 0),
    # proto.hip
    ("SPG_BULLET_HOST_MAX", "LONG", "32", 0),
    ("SPG_FINALS_K", "INT", "8", 0),
    ("SPG_BULLET_DEV", "ON", "on", 0),
    ("SPG_BULLET_AHEAD", "ON", "on", 0),
    ("SPG_BULLET_OVERLAP", "ON", "on", 0),
    ("SPG_DOTLOG_EARLY", "ON", "on", 0),
    ("SPG_DELTA_DEV", "ON", "on", 0),
    ("SPG_DELTA_COMB", "ON", "on", 0),
    # sumcheck.hip
    ("SPG_SC_QUAD_MAX", "LONG", "65536", 0),
    ("SPG_SC_GRID", "INT", "1024", 0),
    ("SPG_EQ_LDS", "ON", "on", 0),
    ("SPG_EQ_MULTI", "ON", "on", 0),
    ("SPG_P1_ROWS", "ON", "on", 0),
    # r1cs.hip, r1cs_tables.hip (the Z fill and k_spmv forms), r1cs_objects.hip (SPG_WIT_IN_PLACE)
    ("SPG_TAPE_AHEAD", "ON", "on", 0),
    ("SPG_SC_FUSE", "ON", "on", 0),
    ("SPG_Z_TILED", "ON", "on", 0),
    ("SPG_Z_SIDE", "ON", "on", 0),
    ("SPG_Z_AFTER", "LONG", "4", 0),
    ("SPG_SPMV_TILED", "ON", "on", 0),
    ("SPG_P1_PAIR", "ON", "on", 0),
    ("SPG_P1_PAIR_MAX", "LONG", "8192", 0),
    ("SPG_SIGMA_AHEAD", "ON", "on", 0),
    ("SPG_Q_BOUND_ALL", "ON", "on", 0),
    ("SPG_P2_PAIR", "ON", "on", 0),
    ("SPG_P2_PAIR_MAX", "LONG", "8192", 0),
    ("SPG_WIT_IN_PLACE", "ON", "on", 0),
    ("SPG_DEBUG_TR", "PRESENT", "off", 1),  # (also verify.hip, snark.hip)
    # snark.hip, verify.hip, rccl.hip
    ("SPG_DEBUG_SNARK", "PRESENT", "off", 1),
    ("SPG_CQ_SIDE", "ON", "on", 1),
    ("SPG_VERIFY_VMSM", "OFF", "off", 0),
    ("SPG_RCCL_TIMEOUT_S", "LONG", "600", 0),
    # hyrax.hip, layers.hip
    ("SPG_HOST_ENC_MAX", "LONG", "384", 0),
    ("SPG_HOST_COMMIT_MAX", "LONG", "0", 0),
    ("SPG_TREE_TOP", "LONG", "1024", 0),
    ("SPG_LAYER_ONEWG", "INT", "512", 0),
    ("SPG_LAYER_EPT", "INT", "2", 0),
    ("SPG_LAYER_QUAD", "ON", "on", 0),
    ("SPG_LAYER_ENDS", "ON", "on", 0),
    ("SPG_LAYER_PAIR", "ON", "on", 0),
    ("SPG_LAYER_TRIPLE", "ON", "on", 0),
    ("SPG_WIDE_MIN", "LONG", "524288", 0),
    ("SPG_PAIR_BS", "INT", "0", 0),
    ("SPG_PAIR_MAX", "LONG", "4096", 0),
    ("SPG_TRIPLE_MAX", "LONG", "384", 0),
    ("SPG_STEP_COSTS", "COSTS", "18,25,30", 0),
    ("SPG_LAYER_DESC_COPY", "PRESENT", "off", 1),
]

# the clamp a site applied to a value that is set, (lo, hi), "-": none; every name not listed here has none
PINNED_CLAMPS = {
    "SPG_BIG_C": ("8", "14"),  # msm_big.hip
    "SPG_BIG_SPT": ("1", "-"),
    "SPG_COMB_C": ("10", "13"),  # comb.hip
    "SPG_COMB_C_WIDE": ("9", "10"),
    "SPG_COMB_C_BIG": ("12", "13"),
    "SPG_VMSM_CH": ("1", "-"),  # msm_var.hip
    "SPG_SC_GRID": ("1", "4096"),  # sumcheck.hip (kScGridMax)
    "SPG_ITEM_K": ("1", "-"),  # msm.hip
    "SPG_SEG_M": ("1", "-"),
    "SPG_FINALS_K": ("1", "-"),  # proto.hip
    "SPG_LAYER_EPT": ("1", "-"),  # layers.hip
    "SPG_RCCL_TIMEOUT_S": ("1", "-"),  # rccl.hip
}

# names that look like knobs in the project's files and are not: error codes, Python-side and build-time names
NOT_KNOBS = {"SPG_OK", "SPG_ERRORS", "SPG_LIB", "SPG_HOSTCHECK_LIB", "SPG_DEVCHECK_LIB", "SPG_BENCH_LAUNCHER",
             "SPG_CHECKED", "SPGH_MAIN"}


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(HC):
        subprocess.check_call(["make", "-s", "-C", PKG, "lib/libspg_hostcheck.so"])
    lib = ctypes.CDLL(HC)
    lib.spgh_knob_table.restype = ctypes.c_size_t
    lib.spgh_knob_table.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    lib.spgh_knob_parse.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.c_long,
                                    ctypes.c_long, ctypes.POINTER(ctypes.c_double)]
    return lib


@pytest.fixture(scope="module")
def table(hc):
    n = hc.spgh_knob_table(None, 0)
    buf = ctypes.create_string_buffer(n)
    assert hc.spgh_knob_table(buf, n) == n
    rows = [line.split("\t") for line in buf.raw.decode().splitlines()]
    assert all(len(r) == 7 for r in rows)
    return [(r[0], r[1], r[2], int(r[5]), r[6], (r[3], r[4])) for r in rows]


def test_names(table):
    names = [r[0] for r in table]
    assert len(set(names)) == len(names), "a name is declared twice"
    external = {"LOCAL_RANK", "LOCAL_WORLD_SIZE"}
    assert external <= set(names)
    for n in set(names) - external:
        assert re.fullmatch(r"SPG_[A-Z0-9_]+", n), n
    assert all(r[4].strip() for r in table), "a row without a description"


def test_defaults(table):
    got = {r[0]: r[1:4] for r in table}
    want = {p[0]: p[1:] for p in PINNED}
    assert len(want) == len(PINNED)
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    wrong = {n: (got[n], want[n]) for n in want if tuple(got[n]) != tuple(want[n])}
    assert not wrong, wrong
    assert set(PINNED_CLAMPS) <= set(want)
    clamps = {r[0]: (r[5], PINNED_CLAMPS.get(r[0], ("-", "-"))) for r in table}
    wrong = {n: c for n, c in clamps.items() if c[0] != c[1]}
    assert not wrong, wrong


NO_LO, NO_HI = -(1 << 63), (1 << 63) - 1
GB = 1 << 30
# (kind, default, lo, hi, {text: expected}); None: unset. Expected: what atoi / atol / atof / sscanf give in the
# expression each read site had ("" and text without digits parse as 0, so they switch an ON knob off)
PARSE_CASES = [
    ("ON", 1, NO_LO, NO_HI, {None: 1, "": 0, "0": 0, "1": 1, "2": 1, "-3": 1, "abc": 0, "0x": 0}),
    ("OFF", 0, NO_LO, NO_HI, {None: 0, "": 0, "0": 0, "1": 1, "2": 1, "-3": 1, "abc": 0}),
    ("PRESENT", 0, NO_LO, NO_HI, {None: 0, "": 1, "0": 1, "1": 1, "2": 1, "-3": 1, "abc": 1}),
    ("INT", 7, NO_LO, NO_HI, {None: 7, "": 0, "0": 0, "1": 1, "2": 2, "-3": -3, "abc": 0, "12abc": 12}),
    # SPG_COMB_C: the default lies outside the clamp and comes back as it stands
    ("INT", 0, 10, 13, {None: 0, "": 10, "0": 10, "1": 10, "2": 10, "-3": 10, "abc": 10, "12": 12, "9": 10, "14": 13,
                        "99": 13}),
    # SPG_BIG_SPT, SPG_ITEM_K, ...: max(1, atoi)
    ("INT", 1, 1, NO_HI, {None: 1, "": 1, "0": 1, "1": 1, "2": 2, "-3": 1, "abc": 1, "100000": 100000}),
    ("INT", 1024, 1, 4096, {None: 1024, "0": 1, "-3": 1, "4096": 4096, "4097": 4096, "2": 2}),  # SPG_SC_GRID
    ("LONG", 64, NO_LO, NO_HI, {None: 64, "": 0, "0": 0, "1": 1, "2": 2, "-3": -3, "abc": 0,
                                "4294967296": 4294967296}),
    ("LONG", 600, 1, NO_HI, {None: 600, "": 1, "0": 1, "1": 1, "2": 2, "-3": 1, "abc": 1, "86400": 86400}),
    # whole gigabytes: the cast to size_t comes before the multiplication; a negative wraps (x86-64's conversion)
    ("GB", 144.0, NO_LO, NO_HI, {None: 144 * GB, "": 0, "0": 0, "1": GB, "2": 2 * GB, "abc": 0, "1.9": GB, "0.5": 0,
                                 "8": 8 * GB, "-3": (1 << 64) - 3 * GB}),
    ("STR", 0, NO_LO, NO_HI, {None: 0, "": 1, "0": 1, "1": 1, "2": 1, "-3": 1, "abc": 1}),
]


@pytest.mark.parametrize("kind,dflt,lo,hi,cases", PARSE_CASES)
def test_parse(hc, kind, dflt, lo, hi, cases):
    d = (ctypes.c_double * 3)(dflt, 0, 0)
    for text, want in cases.items():
        out = (ctypes.c_double * 3)(-1, -1, -1)
        assert hc.spgh_knob_parse(kind.encode(), None if text is None else text.encode(), d, lo, hi, out) == 0
        assert out[0] == want, (kind, text, out[0], want)


def test_parse_step_costs(hc):
    d = (ctypes.c_double * 3)(18, 25, 30)
    cases = {None: (18, 25, 30), "": (18, 25, 30), "abc": (18, 25, 30), "0": (0, 25, 30), "1": (1, 25, 30),
             "2": (2, 25, 30), "-3": (-3, 25, 30), "5,6": (5, 6, 30), "5,6,7": (5, 6, 7), "5,,7": (5, 25, 30),
             "1,1,1": (1, 1, 1), "5,6,7,8": (5, 6, 7)}
    for text, want in cases.items():
        out = (ctypes.c_double * 3)(-1, -1, -1)
        assert hc.spgh_knob_parse(b"COSTS", None if text is None else text.encode(), d, NO_LO, NO_HI, out) == 0
        assert tuple(out) == want, (text, tuple(out), want)
    assert hc.spgh_knob_parse(b"NOPE", b"1", d, NO_LO, NO_HI, (ctypes.c_double * 3)()) == -1


def test_no_drift(table):
    """every SPG_* token in the tests, the scripts and bench.py is a declared knob (or a known non-knob)"""
    declared = {r[0] for r in table}
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "bench.py")]
    files += [f for f in glob.glob(os.path.join(ROOT, "scripts", "*")) if os.path.isfile(f)]
    assert len(files) > 20
    unknown = {}
    for f in files:
        if os.path.abspath(f) == os.path.abspath(__file__):
            continue
        with open(f, errors="replace") as fh:
            for tok in set(re.findall(r"SPGH?_[A-Z0-9_]+", fh.read())):
                if tok in declared or tok in NOT_KNOBS or tok.startswith("SPG_E_") or tok.endswith("_"):
                    continue
                unknown.setdefault(tok, []).append(os.path.relpath(f, ROOT))
    assert not unknown, unknown


# knobs that select no launch form and that no GPU test's environment names, each with its reason. Everything else in
# the table must be named in an environment of tests/test_gpu_*.py or tests/*_cases.py (knobs.hpp: "a new launch form
# adds its row plus an entry in the form list of the matching GPU test").
NOT_A_FORM = {
    "SPG_BIG_PROBE": "debug: per-workgroup timestamps of msm_big on stderr; the results do not depend on it",
    "SPG_COMB_PAD_GB": "cap: its other side (tables that stay packed) runs under SPG_COMB_PAD=0 and the 70 GB table of "
                       "test_comb_big_rule_other_branch",
    "SPG_COPY_TRACE": "trace: counts hipMemcpyAsync calls per source line",
    "SPG_DEBUG_SNARK": "debug: transcript checkpoints on stderr",
    "SPG_DEBUG_TR": "debug: first challenges on stderr",
    "SPG_H2D_TRACE": "trace: one stderr line per streamed upload",
    "SPG_POOL_SPIN_US": "deployment: how long an idle pool worker spins before it parks; no result depends on it",
    "SPG_RCCL_TIMEOUT_S": "deployment: bounded wait of an RCCL exchange (tests/test_gpu_dist.py aborts by failpoint)",
    "SPG_TRACE_EVENTS": "trace: lap ends with their clock times on stderr",
}


def test_every_form_has_a_gpu_test(table):
    """every knob is named in an environment of some GPU test (a quoted name or a NAME= keyword in
    tests/test_gpu_*.py or tests/*_cases.py), or pinned in NOT_A_FORM with its reason"""
    files = glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")) + glob.glob(os.path.join(ROOT, "tests", "*_cases.py"))
    assert len(files) > 20
    text = ""
    for f in files:
        with open(f, errors="replace") as fh:
            text += fh.read()
    names = [r[0] for r in table if r[0].startswith("SPG_")]
    named = {n for n in names if re.search(r"[\"']%s[\"']|\b%s=" % (n, n), text)}
    assert set(NOT_A_FORM) <= set(names), sorted(set(NOT_A_FORM) - set(names))
    assert not (named & set(NOT_A_FORM)), "has a test now; take it out of NOT_A_FORM: %s" % sorted(named & set(NOT_A_FORM))
    missing = sorted(set(names) - named - set(NOT_A_FORM))
    assert not missing, "no GPU test's environment names %s" % missing
    assert all(reason.strip() for reason in NOT_A_FORM.values())


def test_read_sites():
    """knobs.hpp is the only file in csrc/ that reads the environment"""
    hits = []
    for f in sorted(glob.glob(os.path.join(PKG, "csrc", "*"))):
        with open(f, errors="replace") as fh:
            if "getenv(" in fh.read():
                hits.append(os.path.basename(f))
    assert hits == ["knobs.hpp"], hits


def test_documented(table):
    """INTEGRATION.md section 6 has a row for every SPG_* knob, with the table's default"""
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        text = fh.read()
    sec = text[text.index("\n## 6. "):]
    sec = sec[:sec.index("\n## ", 4)] if "\n## " in sec[4:] else sec
    rows = dict(re.findall(r"^\| `([A-Z0-9_]+)` \| ([^|]*?) \|", sec, flags=re.M))
    missing = [r[0] for r in table if r[0].startswith("SPG_") and r[0] not in rows]
    assert not missing, missing
    wrong = {r[0]: (rows[r[0]], r[2]) for r in table if r[0].startswith("SPG_") and rows[r[0]].strip("` ") != r[2]}
    assert not wrong, wrong
    # the heading names the rows that are re-read on every call
    head = sec[:sec.index("\n|")]
    for name, _, _, live, _, _ in table:
        if name.startswith("SPG_"):
            assert (("`%s`" % name) in head) == bool(live), name
