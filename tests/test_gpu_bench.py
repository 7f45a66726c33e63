"""A plain bench.py run on the GPU: the headline line alone, with --steps timed steps, and --dump-outputs holding the
bytes of the proof the line's hash names"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_alone_and_dumps_its_proof(tmp_path):
    # a 2^14-constraint program: the same path as the headline, set up in about a second
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--log-proofs", "3",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["constraints_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    # what --full adds stays out of a plain run
    for k in ("kernels", "roofline", "cpu_baseline", "transcript_mode", "verify_ms", "config2_msm", "config5_spark"):
        assert k not in d
    assert os.listdir(tmp_path / "out") == ["proof.npy"]
    proof = np.load(tmp_path / "out" / "proof.npy")
    assert proof.dtype == np.float32
    assert hashlib.sha256(proof.astype(np.uint8).tobytes()).hexdigest().startswith(d["proof_sha256"])
