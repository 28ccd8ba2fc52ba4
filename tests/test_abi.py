"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol include/mlmap_hip.h
declares, fails loudly without a GPU, and the C++ facade compiles against the header."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mlm_[A-Za-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported():
    from mlmapping_amd.mlmap import ABI_SYMBOLS, load_library

    lib = load_library()
    decl = _declared()
    assert len(decl) >= 25
    for s in decl:
        assert hasattr(lib, s), f"{s} declared in include/mlmap_hip.h but not exported"
    assert sorted(ABI_SYMBOLS) == decl, "python binding and header disagree on the ABI surface"
    assert lib.mlm_abi_version() == 6


def test_no_cpu_fallback():
    """Without a GPU the product path must fail loudly (never route to the oracle or any CPU path)."""
    import ctypes

    from mlmapping_amd.config import S1
    from mlmapping_amd.mlmap import MLMap, MlmError, load_library

    lib = load_library()
    n = ctypes.c_int(0)
    hip = ctypes.CDLL(None)  # the HIP runtime the library is bound to (already in the process, see mlmap.load_library)
    if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(MlmError):
        MLMap(S1)


def test_product_does_not_import_oracle():
    """Nothing under mlmapping_amd/ or include/ may reference the oracle."""
    bad = []
    for base in ("mlmapping_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".h", ".hpp", ".hip", ".cpp")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    if "mlo_" in txt or "libmlmap_oracle" in txt or re.search(r"(from|import)\s+oracle", txt):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_facade_compiles(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "mlmap_facade.hpp"\nint main(){ mlmap_hip::mlmap m; (void)m; return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_knob_values_the_kernels_cannot_run_are_refused():
    """mlm_debug_set refuses launch geometries no kernel can run (MLM_ERR_INVALID) and accepts the ones they can: block sizes of whole
    waves up to __launch_bounds__(256) (k_expand_nodes / k_sort_contribs take lane = threadIdx.x & 63, wave = threadIdx.x >> 6),
    the three tiles of k_bin_points, grids of one workgroup or more.  Host only: nothing here is launched."""
    from mlmapping_amd.mlmap import MLM_OK, load_library
    from tests.util import BLOCK_KNOBS, GRID_KNOBS

    L = load_library()
    ERR_INVALID = -1
    try:
        for name in BLOCK_KNOBS:
            for v in (64, 128, 192, 256):
                assert L.mlm_debug_set(name.encode(), v) == MLM_OK, (name, v)
            for v in (-64, 0, 1, 32, 63, 65, 96, 100, 160, 255, 257, 320, 512, 1024, 1 << 40):
                assert L.mlm_debug_set(name.encode(), v) == ERR_INVALID, (name, v)
        for v in (256, 512, 1024):
            assert L.mlm_debug_set(b"bin_block", v) == MLM_OK, v
        for v in (-256, 0, 1, 64, 128, 255, 257, 384, 511, 768, 1023, 1025, 2048):
            assert L.mlm_debug_set(b"bin_block", v) == ERR_INVALID, v
        for name in GRID_KNOBS:
            for v in (1, 2, 3, 7, 13, 256, 4096, 1 << 20):
                assert L.mlm_debug_set(name.encode(), v) == MLM_OK, (name, v)
            for v in (0, -1, -256, (1 << 20) + 1, 1 << 31, 1 << 40):
                assert L.mlm_debug_set(name.encode(), v) == ERR_INVALID, (name, v)
        for name in ("cu_split", "cu_reserve"):  # (the upper bound is the CU count: mlm_create checks it, tests/test_gpu_geometry.py)
            for v in (0, 8, 16, 255):
                assert L.mlm_debug_set(name.encode(), v) == MLM_OK, (name, v)
            for v in (-1, -16, 1 << 40):
                assert L.mlm_debug_set(name.encode(), v) == ERR_INVALID, (name, v)
        assert L.mlm_debug_set(b"no_such_grid", 1) == ERR_INVALID  # (names outside kKnobNames: refused whatever the value)
    finally:
        L.mlm_debug_reset()
