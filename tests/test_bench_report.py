"""bench.py's report helpers on a synthetic profile (no GPU): the roofline objects and the kernel table read the
per-kernel tuples spg.Context.prof_read(ops=True) returns -- (launches, us, bytes, madds, Fq products) -- whatever
mix of modelled quantities a kernel carries; and its timing loop, output dump and option defaults"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def synthetic(bench):
    p = bench.Prof({
        "spark_layer_round": (100, 1000.0, 1.5e8, 0.0, 4.0e7),     # bytes + Fq products
        "msm_bullet_round": (50, 800.0, 5.0e7, 2.5e5, 0.0),         # bytes + madds
        "msm_comb": (2, 5000.0, 0.0, 1.0e8, 0.0),                   # madds only
        "sc_phase1_fold_eval": (10, 900.0, 6.0e8, 0.0, 1.2e8),
        "eq_table": (20, 100.0, 1.0e6, 0.0, 0.0),
    })
    p.busy_us = 7000.0
    p.busy_resident_us = 7000.0
    return p


def test_rooflines_read_five_field_tuples(bench):
    prof = synthetic(bench)
    roof, h, v = bench.rooflines(prof)
    assert h["kernel"] == "spark_layer_round" and h["bound"] == "hbm"
    assert v["kernel"] == "msm_comb" and v["bound"] == "valu"
    assert roof is v  # the kernel with the most device time among the modelled ones
    assert abs(v["achieved"] - 1.0e8 / 5000e-6) < 1.0
    f = bench.roofline_fq(prof)
    assert f["kernel"] == "spark_layer_round" and f["bound"] == "valu_fq"
    assert abs(f["achieved"] - 4.0e7 / 1000e-6) < 1.0
    assert 0 < f["frac"] < 1 and f["hbm_frac"] > 0


def test_rooflines_on_four_field_tuples(bench):
    # a library built before the Fq-product counter reports four fields
    prof = bench.Prof({k: v[:4] for k, v in synthetic(bench).items()})
    roof, h, v = bench.rooflines(prof)
    assert roof is not None and h is not None and v is not None
    assert bench.roofline_fq(prof) is None


class OneRank:
    """what timed() / dump_outputs() use of bench.Env, for one rank without a device"""
    rank, world = 0, 1

    def sync(self):
        pass

    def max_over_ranks(self, x):
        return x


def test_timed_runs_the_steps_asked_for_and_returns_the_last_result(bench):
    calls = []

    def step():
        calls.append(len(calls))
        return bytes([calls[-1]])

    dt, laps, hashes, last = bench.timed(OneRank(), step, steps=5, warmup=2)
    assert len(calls) == 7 and len(laps) == 5 and len(hashes) == 5
    assert last == bytes([6]) and dt >= sum(laps) > 0


def test_dump_outputs_writes_float32_arrays_of_the_bytes(bench, tmp_path):
    import numpy as np

    raw = bytes(range(256)) * 3
    bench.dump_outputs(OneRank(), str(tmp_path / "d"), proof=raw, rows=np.frombuffer(raw[:64], dtype=np.uint8))
    got = np.load(tmp_path / "d" / "proof.npy")
    assert got.dtype == np.float32 and got.shape == (768,)
    assert got.astype(np.uint8).tobytes() == raw
    assert np.load(tmp_path / "d" / "rows.npy").astype(np.uint8).tobytes() == raw[:64]


def test_full_is_off_by_default(bench, monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 4
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


def test_kernel_table(bench):
    t = bench.kernel_table(synthetic(bench), steps=2, top=3)
    assert list(t) == ["msm_comb", "spark_layer_round", "sc_phase1_fold_eval"]
    assert t["spark_layer_round"]["fq_products_per_s"] > 0 and t["msm_comb"]["madds_per_s"] > 0
    assert t["msm_comb"]["GBps"] is None
