"""The host flattener of the preemption tables' NRT side table under AddressSanitizer and UBSan (no GPU): tests/cpp/flatten_preempt_nrt_main.cc,
a program with its own main, is built together with the host sources it calls and run on a seeded snapshot whose output arrays are
exactly as large as include/spx.h states."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "scheduler-plugins_amd" / "host"
SOURCES = [ROOT / "tests" / "cpp" / "flatten_preempt_nrt_main.cc", HOST / "flatten_preempt_nrt.cc", HOST / "flatten_nrt.cc", HOST / "nrt_preemption.cc"]


def test_flattener_runs_clean_under_asan_and_ubsan():
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(parents=True, exist_ok=True)
    exe = out / "flatten_preempt_nrt_sanitized"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}",
           *map(str, SOURCES), "-lpthread", "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "nodes checked against the eviction simulation" in r.stdout
