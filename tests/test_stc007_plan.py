"""The host's decisions in the STC-007 chain speculation (sdvpcmdecoder_amd/csrc/stc007_chain_plan.h) without a tape: tests/emu/stc007_plan_check.cpp feeds the
plan flag bytes, give-up signatures and reference levels made by hand and checks the round's lists against the rules the plan's comments state - a leader
needs two followers, a held crowd waits for its leader's sweep, a run of links that moved has one anchor.  Host code only: built here with g++ under
AddressSanitizer and UBSan as a program of its own, on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_fed_by_hand(tmp_path):
    exe = str(tmp_path / "stc007_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-w", "-o", exe,
                    os.path.join(ROOT, "tests", "emu", "stc007_plan_check.cpp")], check=True, cwd=os.path.join(ROOT, "tests", "emu"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PLAN_OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
