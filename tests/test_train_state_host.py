"""The byte format of an exported training state (fsrl_amd/csrc/train_state.hpp: writer, reader, validator) as a stand-alone program:
tests/host/train_state_sim.cpp, its own process, nothing preloaded, nothing loaded into Python, built with the address / undefined-
behaviour sanitizers.  The header parses bytes that come from a file, so the program hands it what a damaged or foreign file can
hold: every prefix, a flipped bit at every position, lengths past the end and below zero, unknown / duplicate / missing sections,
every fingerprint field changed in turn, sub-buffer books no sequence of pushes produces."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "train_state_sim.cpp")


def test_train_state_format_survives_hostile_input(tmp_path):
    exe = str(tmp_path / "train_state_sim")
    # -static-lib*san: see tests/test_resident_ring.py (a dynamically linked sanitizer runtime must be the first library loaded)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    oks = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert oks == ["round_trip", "prefixes", "bit_flips", "lengths", "tags", "header", "fingerprint", "store_and_host", "writer_bounds"], out.stdout
    lines = {ln.split()[1]: ln for ln in out.stdout.splitlines() if ln.startswith("ok ")}
    n = int(lines["round_trip"].split("bytes=")[1].split()[0])
    assert lines["prefixes"] == "ok prefixes refused=%d" % n                 # lengths 0 .. n - 1
    assert lines["bit_flips"] == "ok bit_flips refused=%d" % (8 * n)         # every bit of every byte
    assert lines["fingerprint"] == "ok fingerprint fields=20"
