"""What the host engines rely on in namespace rt (sdvpcmdecoder_amd/csrc/runtime.inc), in the form the emulator build gets: tests/emu/rt_shim_check.cpp checks
the grow-only buffers and their failure rule, the split of a grid stride into frames, rows and slots, the emulator's launch sizes, the two kinds of kernel
launch, and that events, timers and side streams do nothing and allocate nothing.  Host code only: built here with g++ under AddressSanitizer and UBSan as
a program of its own, on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_runtime_shim_in_its_emulator_form(tmp_path):
    exe = str(tmp_path / "rt_shim_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-w", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "rt_shim_check.cpp")], check=True, cwd=os.path.join(ROOT, "tests", "emu"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RT_SHIM_OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
