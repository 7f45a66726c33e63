"""Reader safety of the oracle's bincode reader De: tests/de_check/de_check.cpp, a stand-alone program built with
ASan + UBSan against the oracle headers, parses the honest small-case proof, every truncation of it at a field
boundary and the proof with each Vec length set to 0, length + 1 and 2^63, and must find each of these malformed
without a sanitizer report. It runs as its own process on the CPU; nothing is preloaded or loaded into Python."""
import os
import subprocess

from r1cs_cases import SNARK_CASES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_de_check_under_asan_ubsan(oracle, tmp_path):
    import workload
    from proof_layout import snark_proof_fields_typed

    proof, rc = oracle.snark_prove(workload.SnarkWorkload(**SNARK_CASES["b2_x32_q2"]), workload.tape_seed())
    assert rc == 0
    (tmp_path / "proof.bin").write_bytes(proof)
    typed = snark_proof_fields_typed(proof)
    lines = [f"b {s}" for _, s, _, _ in typed] + [f"l {s}" for _, s, _, k in typed if k == "len"]
    assert len(lines) > 3000
    (tmp_path / "offsets.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "de_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-march=x86-64-v2", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                           os.path.join(HERE, "de_check", "de_check.cpp")])
    r = subprocess.run([exe, str(tmp_path / "proof.bin"), str(tmp_path / "offsets.txt")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
