#!/usr/bin/env python3
"""Generates the per-line STC-007 golden fixtures (stc_lines_mode<m>.npz) by running the REAL reference (oracle/_ref/libsdvref.so:
Binarizer::processLine with an STC007Line output, a Binarizer per line, ref_bin_process) on the lines of tests/test_stc_lines.py.
Runs only where the reference build exists (oracle/Makefile.ref).

Each fixture: sha256 of the input luma rows (regenerated from the seed by the test) and the expected line records (48 bytes each) of
two runs: every line cold (`cold`) and every line preset with what a worker that plays the lines in order hands on (`behind`)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libs  # noqa: E402
import test_stc_lines as t  # noqa: E402

if __name__ == "__main__":
    ref = libs.load_ref()
    rows = t._lines()
    for mode in t.GOLDEN_MODES:
        cold = t._per_line(ref, "ref_bin_", rows, None, mode)
        behind = t._per_line(ref, "ref_bin_", rows, t._states_behind(cold, mode), mode)
        path = os.path.join(HERE, "stc_lines_mode%d.npz" % mode)
        np.savez_compressed(path, input_sha256=hashlib.sha256(rows.tobytes()).hexdigest(),
                            cold=cold.view(np.uint8).reshape(len(cold), 48), behind=behind.view(np.uint8).reshape(len(behind), 48))
        print(f"mode {mode}: {len(rows)} lines, {int((cold['flags'] & t.LF_CRC_VALID != 0).sum())} / "
              f"{int((behind['flags'] & t.LF_CRC_VALID != 0).sum())} with a valid CRC, {os.path.getsize(path)} bytes")
