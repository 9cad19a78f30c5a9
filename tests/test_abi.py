"""The C-ABI library loads and exports every symbol include/sdvpcm.h declares (no compute without a GPU)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "sdvpcm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sdv_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    for s in ("sdv_engine_create", "sdv_engine_destroy", "sdv_binarize_frames", "sdv_set_mode", "sdv_set_bin_preset",
              "sdv_last_error"):
        assert s in syms


def test_product_library_exports_all_symbols():
    from sdvpcmdecoder_amd import build as b
    path = b.build_hip()
    lib = C.CDLL(path)
    for s in declared_symbols():
        assert hasattr(lib, s), f"libsdvpcm_hip.so does not export {s}"
    hdr = open(os.path.join(ROOT, "include", "sdvpcm.h")).read()
    assert lib.sdv_abi_version() == int(re.search(r"#define SDV_ABI_VERSION (\d+)", hdr).group(1))


def test_emulator_library_exports_all_symbols():
    from sdvpcmdecoder_amd import build as b
    lib = C.CDLL(b.build_emu())
    for s in declared_symbols():
        assert hasattr(lib, s), f"libsdvpcm_emu.so does not export {s}"


# ---- sdvpcmdecoder_amd/abi.py against the header: parameter lists by parsing it, layouts and constants through the C compiler ----
C_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "double": C.c_double, "uint8_t": C.c_uint8, "int16_t": C.c_int16,
             "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


def header_prototypes():
    """[(return type, name, [parameter, ...])] in the order of the header."""
    src = open(os.path.join(ROOT, "include", "sdvpcm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = "\n".join(ln for ln in src.split("\n") if not ln.lstrip().startswith("#"))
    src = re.sub(r"\{[^{}]*\}", "{}", src)              # struct and enum bodies (one pass: extern "C" { stays open)
    protos = []
    for stmt in src.split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]*?)\b(sdv_\w+)\s*\(([^()]*)\)\s*", stmt.split("}")[-1])
        if m:
            params = [p.strip() for p in m.group(3).split(",")]
            protos.append((" ".join(m.group(1).split()), m.group(2), [] if params == ["void"] else params))
    return protos


def _pointee(decl):
    """'const sdv_bin_preset *p' -> 'sdv_bin_preset'; 'double c[3]' -> 'double'; a scalar -> None"""
    if "*" in decl:
        return decl.split("*")[0].replace("const", "").strip()
    return decl.replace("const", "").split()[0] if "[" in decl else None


def test_prototypes_match_the_header():
    from sdvpcmdecoder_amd import abi
    protos = header_prototypes()
    assert len(protos) == len(declared_symbols()) == 104
    assert [name for _, name, _ in protos] == list(abi.PROTOTYPES), "the table follows the header's order and holds nothing else"
    assert not set(abi.DEV_PROTOTYPES) & set(abi.PROTOTYPES)
    for ret, name, params in protos:
        restype, argtypes = abi.PROTOTYPES[name]
        if "*" in ret:
            assert restype is (C.c_char_p if "char" in ret else C.c_void_p), name
        else:
            assert restype is (None if ret == "void" else C_SCALARS[ret]), name
        assert len(argtypes) == len(params), name
        for decl, got in zip(params, argtypes):
            to = _pointee(decl)
            if to is None:
                assert got is C_SCALARS[" ".join(decl.split()[:-1])], (name, decl)
            else:
                typed = C_SCALARS.get(to) or abi.RECORDS.get(to)
                assert got is C.c_void_p or (typed is not None and got is C.POINTER(typed)), (name, decl)


_probe_cache = []


def _probe(tmp_path_factory):
    """sizeof / offsetof of every member of every record of abi.RECORDS, and the value of every constant, as the C compiler sees the header."""
    import subprocess
    from sdvpcmdecoder_amd import abi
    if not _probe_cache:
        body = []
        for t, cls in abi.RECORDS.items():
            body.append('printf("%s %%zu\\n", sizeof(%s));' % (t, t))
            for m, _ in cls._fields_:
                body.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (t, m, t, m, t, m))
        for n in abi.CONSTANTS:
            body.append('printf("SDV_%s %%lld\\n", (long long)SDV_%s);' % (n, n))
        d = tmp_path_factory.mktemp("abi_probe")
        (d / "probe.c").write_text('#include <stdio.h>\n#include "sdvpcm.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(d / "probe"), str(d / "probe.c")])
        out = subprocess.check_output([str(d / "probe")], text=True)
        _probe_cache.append({ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in out.splitlines()})
    return _probe_cache[0]


def test_record_layouts_match_the_compiler(tmp_path_factory):
    import numpy as np
    from sdvpcmdecoder_amd import abi
    c = _probe(tmp_path_factory)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdvpcm.h")).read(), flags=re.S)
    typedefs = set(re.findall(r"\}\s*(sdv_\w+)\s*;", hdr))
    assert typedefs == set(abi.RECORDS), "every POD typedef of the header has its record"
    for t, cls in abi.RECORDS.items():
        dt = np.dtype(cls)
        assert (C.sizeof(cls),) == c[t] == (dt.itemsize,), t
        for m, _ in cls._fields_:
            f = getattr(cls, m)
            assert (f.offset, f.size) == c[t + "." + m] == (dt.fields[m][1], dt.fields[m][0].itemsize), (t, m)
    assert abi.BIN_STATE_SHORT_DTYPE.itemsize == c["sdv_bin_state"][0]
    assert [abi.BIN_STATE_SHORT_DTYPE.fields[n] for n in abi.BIN_STATE_SHORT_DTYPE.names] == [abi.BIN_STATE_DTYPE.fields[n] for n in abi.BIN_STATE_DTYPE.names]


def test_constants_match_the_compiler(tmp_path_factory):
    from sdvpcmdecoder_amd import abi
    c = _probe(tmp_path_factory)
    for n, v in abi.CONSTANTS.items():
        assert (v,) == c["SDV_" + n] and getattr(abi, n) == v, n


def test_the_abi_is_stated_in_one_place_only():
    """No prototype of an sdv_* symbol and no dtype literal of a record outside sdvpcmdecoder_amd/abi.py (and the entry script), and
    every handle of the library that tests and tools open themselves goes through a bind() where it is opened."""
    import glob
    from sdvpcmdecoder_amd import abi
    records = {tuple(n for n, _ in cls._fields_) for cls in abi.RECORDS.values()}
    for path in sorted(glob.glob(os.path.join(ROOT, "sdvpcmdecoder_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        if os.path.basename(path) == "abi.py":
            continue
        text = open(path).read()
        lines = text.split("\n")
        for i, ln in enumerate(lines):
            if re.search(r"\.(argtypes|restype)\s*(=|,)", ln) and not re.search(r"\b(orc|ref)_", ln):
                ctx = "\n".join(lines[max(0, i - 3):i + 1]) if "getattr(" in ln else ln      # the names a getattr(lib, nm) loop runs over
                assert "sdv_" not in ctx, "%s:%d sets a prototype of the C-ABI" % (path, i + 1)
            if "CDLL(" in ln and re.search(r"build_hip|build_emu|libsdvpcm|_name\b", ln) and os.path.basename(path) != "test_abi.py":
                assert re.search(r"bind\w*\(|EmuEngine\(", ln), "%s:%d calls through a handle nothing has typed" % (path, i + 1)
        if os.sep + "tools" + os.sep not in path:
            for lit in re.findall(r"np\.dtype\(\[(.*?)\]\)", text, flags=re.S):
                assert tuple(re.findall(r"\(\"(\w+)\"", lit)) not in records, "%s restates a record of the C-ABI" % path


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sdvpcmdecoder_amd import Engine
    with pytest.raises(RuntimeError, match="no HIP device|sdv_engine_create failed"):
        Engine(0)


def test_product_does_not_reference_oracle():
    """The product sources must not include or link anything under oracle/ or the emulator."""
    pkg = os.path.join(ROOT, "sdvpcmdecoder_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".inc", ".cpp")) and f != "build.py":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "liborc" not in text and "oracle/" not in text.replace("(see oracle/", ""), f
                assert "hip_emu.h" not in text or f == "stc007_device.h" or f == "engine.inc", f


def test_header_is_plain_c(tmp_path):
    """The boundary is a C ABI: the header must compile as C99 and as C++ on its own, and the PODs must have the documented sizes."""
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include "sdvpcm.h"\n'
                   '#define CHECK(t, n) typedef char check_##t[(sizeof(t) == (n)) ? 1 : -1]\n'
                   'CHECK(sdv_line_rec, 48); CHECK(sdv_frame_stats, 32); CHECK(sdv_v2d_state, 120); CHECK(sdv_deint_line, 24);\n'
                   'CHECK(sdv_block_rec, 72); CHECK(sdv_sample_pair, 12); CHECK(sdv_frame_asm, 64); CHECK(sdv_stitch_settings, 16); CHECK(sdv_audio_purge, 16);\n'
                   'CHECK(sdv_pcm1_block_rec, 576); CHECK(sdv_pcm1_asm_line_rec, 16); CHECK(sdv_pcm16x0_block_rec, 32); CHECK(sdv_asm_line_rec, 32);\n'
                   'int main(void) { sdv_engine *e = sdv_engine_create(0); sdv_engine_destroy(e); return 0; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)])


# ---- the boundary driven from plain C++ host code (examples/decode_tape.cpp): no Python, no torch in the process that decodes ----
def test_cpp_example_builds():
    from sdvpcmdecoder_amd import build as b
    assert os.path.exists(b.build_example())


@pytest.mark.gpu
def test_cpp_host_program_matches_reference_golden(tmp_path):
    """decode_tape stc007: luma file -> sdv_binarize_frames(NEW_FILE | END_FILE) -> sdv_stitch_frames, written by a C++ program that
    links libsdvpcm_hip.so; compared with the real reference's output for the same file (tests/golden/e2e_ntsc_file.npz)."""
    import subprocess
    import numpy as np
    from sdvpcmdecoder_amd import build as b
    import test_stitch_kernel as tsk
    exe = b.build_example()
    luma, z, want_p, want_f = tsk._e2e_fixture()
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    out = subprocess.run([exe, "stc007", str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "pairs.out"), str(tmp_path / "frames.out")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert (tmp_path / "pairs.out").read_bytes() == want_p.tobytes()
    assert (tmp_path / "frames.out").read_bytes() == want_f.tobytes()


@pytest.mark.gpu
def test_cpp_host_program_pcm1_matches_reference_golden(tmp_path):
    import subprocess
    import numpy as np
    import pcm1_api as p1
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example()
    z = np.load(os.path.join(ROOT, "tests", "golden", "pcm1_file_marks.npz"))
    recs, st = p1.make_input("file_marks")
    (tmp_path / "lines.raw").write_bytes(recs.tobytes())
    out = subprocess.run([exe, "pcm1", str(tmp_path / "lines.raw"), str(tmp_path / "pairs.out"), str(tmp_path / "frames.out")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert (tmp_path / "pairs.out").read_bytes() == np.ascontiguousarray(z["pairs"]).tobytes()
    assert (tmp_path / "frames.out").read_bytes() == np.ascontiguousarray(z["frames"]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["si", "ei"])
def test_cpp_host_program_pcm16x0_matches_reference_golden(fmt, tmp_path):
    """decode_tape pcm16x0: luma file -> sdv_pcm16x0_binarize_frames(NEW_FILE | END_FILE) -> sdv_pcm16x0_stitch_frames from plain C++;
    compared with the real reference's two workers on the same file (tests/golden/e2e_pcm16x0_*.npz)."""
    import subprocess
    import numpy as np
    from sdvpcmdecoder_amd import build as b
    import test_pcm16 as t16
    exe = b.build_example()
    luma, audio, z, want_p, want_f = t16._e2e_fixture(fmt == "ei")
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    out = subprocess.run([exe, "pcm16x0", str(tmp_path / "luma.raw"), str(w), str(h), str(n), fmt, str(tmp_path / "pairs.out"), str(tmp_path / "frames.out")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert (tmp_path / "pairs.out").read_bytes() == want_p.tobytes()
    assert (tmp_path / "frames.out").read_bytes() == want_f.tobytes()


@pytest.mark.gpu
def test_cpp_host_program_writes_the_reference_wav(tmp_path):
    """decode_tape wav: luma file -> binarize -> stitch -> sdv_audio_process -> sdv_wav_pack / sdv_wav_header from plain C++; the file equals the
    one the real reference's SamplesToWAV wrote at the end of its own chain (tests/golden/e2e_ntsc_file_audio.npz)."""
    import subprocess
    import numpy as np
    from sdvpcmdecoder_amd import build as b
    import test_stitch_kernel as tsk
    import test_audio as ta
    exe = b.build_example()
    luma, _, _, _ = tsk._e2e_fixture()
    z, _, wavs = ta._e2e_audio_fixture()
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    out = subprocess.run([exe, "wav", str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out.wav")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert (tmp_path / "out.wav").read_bytes() == wavs[0]
