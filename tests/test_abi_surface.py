"""CPU: the C-ABI shared object loads (no GPU needed) and exports exactly the entry points include/*.h declare (ddpm_hip.h = the
interface that replaces the reference's ATen calls; ddpm_hip_debug.h = instrumentation and test hooks, none of which the product path needs);
the ctypes table binds every one of them with the right arity."""
import ctypes
import os
import re

import pytest

from ddpm_torch import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ddpm_hip.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "ddpm_hip_debug.h")          # instrumentation / measurement / test hooks: a separate header


def declared(paths=(HEADER, DEBUG_HEADER)):
    src = "".join(re.sub(r"/\*.*?\*/", "", open(p).read(), flags=re.S) for p in paths)
    out = {}
    for m in re.finditer(r"\b(?:int|long long|void\s*\*|const char\s*\*)\s*(ddpm_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = [a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        out[m.group(1)] = len(args)
    return out


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
def test_library_exports_every_declared_symbol():
    decl = declared()
    assert len(decl) >= 25
    handle = ctypes.CDLL(_hip.LIB_PATH)
    for name in decl:
        assert hasattr(handle, name), f"{name} declared in ddpm_hip.h but not exported"
    assert set(decl) == set(_hip.PROTOTYPES), set(decl) ^ set(_hip.PROTOTYPES)
    for name, nargs in decl.items():
        assert len(_hip.PROTOTYPES[name]) == nargs, (name, nargs, len(_hip.PROTOTYPES[name]))
    _hip.lib()
    # the interface header carries no instrumentation: every hook lives in the debug header
    hooks = {"ddpm_conv2d_variant", "ddpm_conv2d_wgrad_variant", "ddpm_gemm_variant", "ddpm_mfma_probe", "ddpm_copy_probe", "ddpm_dropout_mask",
             "ddpm_conv3x3_pc_last_fault", "ddpm_set_reserved_cus", "ddpm_get_reserved_cus"}
    assert hooks <= set(declared((DEBUG_HEADER,))) and not hooks & set(declared((HEADER,)))


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
def test_argument_validation_returns_status_codes_without_a_gpu():
    lib = _hip.lib()
    # null pointers / bad shapes are rejected on the host before any launch
    assert lib.ddpm_q_sample(0, 0, 0, 0, 0, 0, 1, 1, 10, 0) == 5
    assert lib.ddpm_gn_workspace_floats(2, 64, 100, 32, 1) == -1          # 100 channels not divisible by 32
    assert lib.ddpm_gn_workspace_floats(2, 64, 128, 32, 1) > 0
    with pytest.raises(RuntimeError, match="null pointer"):
        _hip.call("ddpm_silu_fwd", 0, 0, 10, 0)
    # maximum sizes: the kernels address an operand with 32-bit byte offsets, so a tensor of 2 GiB or more is refused on the host
    # (32 x 32 x 384 channels bf16: B = 4096 is 3 GiB; B = 2048 = 1.5 GiB passes validation).  Only the refused size goes through the
    # launching entry point: a size that passes would launch a kernel on these fake addresses wherever a GPU is present, so it is put to
    # the same dispatch with launching switched off (ddpm_conv2d_variant: the id of the kernel it would run, or -status)
    fake = 0x10000
    conv = lambda B: lib.ddpm_conv2d_nhwc(fake, 384, fake, fake, 128, 0, 0, 0, 0, 0, B, 32, 32, 384, 32, 32, 128, 3, 3, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0)
    dry = lambda B: lib.ddpm_conv2d_variant(384, 128, B, 32, 32, 384, 32, 32, 128, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 0)
    assert conv(4096) == 1 and dry(4096) == -1 and dry(2048) >= 0


QUERIES = {"ddpm_wgrad_effective_splits", "ddpm_conv3x3_wgrad_splits", "ddpm_conv1x1_wgrad_splits", "ddpm_gn_workspace_floats",
           "ddpm_conv2d_variant", "ddpm_conv2d_wgrad_variant", "ddpm_gemm_variant", "ddpm_conv3x3_pc_last_fault", "ddpm_set_reserved_cus",
           "ddpm_get_reserved_cus", "ddpm_mt_sumsq_slots", "ddpm_conv3x3_wgrad_variant", "ddpm_wgrad3x3_ws_last_fault"}


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
def test_plan_executor_knows_every_launching_entry_point_with_the_declared_arity():
    """csrc/plan.hip generates its call thunks from the header's declarations; the ctypes table is what the recorder converts arguments
    with — the two must agree for every entry point a step can record."""
    lib = _hip.lib()
    for name, argtypes in _hip.PROTOTYPES.items():
        arity = lib.ddpm_plan_entry_arity(name.encode())
        if name in QUERIES or name.startswith("ddpm_plan_"):
            assert arity == -1, name                               # pure queries / the plan API itself enqueue nothing: not recordable
        else:
            assert arity == len(argtypes), (name, arity, len(argtypes))


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
def test_plan_api_validates_on_the_host():
    lib = _hip.lib()
    h = ctypes.c_void_p(lib.ddpm_plan_create())
    assert h.value
    words = (ctypes.c_ulonglong * 4)(0, 0, 10, 0)
    as_ptr = ctypes.cast(words, ctypes.c_void_p)
    assert lib.ddpm_plan_append(h, b"ddpm_silu_fwd", as_ptr, 4) == 0            # first entry
    assert lib.ddpm_plan_append(h, b"ddpm_silu_fwd", as_ptr, 3) == -1           # wrong argument count
    assert lib.ddpm_plan_append(h, b"ddpm_no_such_entry", as_ptr, 4) == -1
    assert lib.ddpm_plan_append(h, b"ddpm_gemm_variant", as_ptr, 4) == -1       # a query is not a launch
    assert lib.ddpm_plan_entries(h) == 1 and lib.ddpm_plan_segments(h) == 1
    assert lib.ddpm_plan_cut(h) == 0 and lib.ddpm_plan_segments(h) == 1
    assert lib.ddpm_plan_append(h, b"ddpm_silu_fwd", as_ptr, 4) == 1 and lib.ddpm_plan_segments(h) == 2
    # running it calls ddpm_silu_fwd(NULL, NULL, 10, stream 0): rejected on the host (null pointer = 5) before any launch, and reported
    assert lib.ddpm_plan_run(h, 0) == 5
    idx = ctypes.c_int(-1)
    name = lib.ddpm_plan_failed_entry(h, ctypes.cast(ctypes.pointer(idx), ctypes.c_void_p))
    assert name == b"ddpm_silu_fwd" and idx.value == 0
    assert lib.ddpm_plan_run(h, 7) == 1                                         # no such segment
    assert lib.ddpm_fill_zero(0, 16, 0) == 5 and lib.ddpm_fill_zero(0, 0, 0) == 0 and lib.ddpm_fill_zero(0, -1, 0) == 1
    assert lib.ddpm_plan_destroy(h) == 0


PKG = os.path.join(ROOT, "ddpm-torch_amd")
RETIRED_MACROS = ("PC_ABL_", "PC_DEFAULT_OFF", "GN_ABL_", "GABL_")


def _sources(top, suffixes):
    for d, _, files in os.walk(top):
        for f in files:
            if f.endswith(suffixes):
                yield os.path.join(d, f)


def test_every_environment_switch_is_in_the_integration_table_and_no_ablation_macro_is_back():
    """The project's switches are the rows of INTEGRATION.md's "Environment" table, no more and no fewer: every DDPM_* name a getenv( call
    under csrc/ or an environ read in the package mentions is documented there, and every documented name is still read.  A kernel
    experiment is a second build of the library (DDPM_HIP_LIB), not a new branch in the product's dispatch."""
    read = set()
    for path in _sources(os.path.join(PKG, "csrc"), (".hip", ".h", ".py")):
        for line in open(path):
            if "getenv(" in line or "environ" in line:
                read |= set(re.findall(r"DDPM_[A-Z0-9_]+", line.split("//")[0]))
    for path in _sources(PKG, (".py",)):
        for line in open(path):
            if "environ" in line:
                read |= set(re.findall(r"DDPM_[A-Z0-9_]+", line.split("#")[0]))
    section = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("\n## 4. Environment", 1)[1].split("\n## ", 1)[0]
    table = set()
    for row in section.splitlines():
        if row.startswith("| `"):
            table |= set(re.findall(r"`(DDPM_[A-Z0-9_]+)`", row.split("|")[1]))
    assert len(table) >= 10
    assert read == table, (sorted(read - table), sorted(table - read))
    for path in _sources(os.path.join(PKG, "csrc"), (".hip", ".h")):
        src = open(path).read()
        assert not [m for m in RETIRED_MACROS if m in src], path


PRIMITIVES = ("BUF_OOB", "buffer_rsrc", "lds_addr", "LDS_DMA16", "wait_vm", "lds_rd16", "lds_rd_tr", "lds_wait", "lds_wait_n", "static_for",
              "xcd_logical_id", "lds_wait_all_ge", "lds_wait_ge", "lds_signal", "lds_publish")


def test_gfx950_device_primitives_live_in_the_shared_header_only():
    """The low-level building blocks of the LDS-DMA kernels are written once, in csrc/gfx950.h: outside it no .hip file spells the
    LDS-DMA builtin or the out-of-range offset, the buffer-descriptor builtin appears exactly once (gemm.hip's slab_rs, built without
    readfirstlane on purpose), and no file defines a second copy of a primitive the header defines (once)."""
    csrc = os.path.join(PKG, "csrc")
    hips = {os.path.basename(p): open(p).read() for p in _sources(csrc, (".hip",))}
    assert len(hips) >= 14
    assert not [f for f, src in hips.items() if "__builtin_amdgcn_raw_ptr_buffer_load_lds" in src]
    assert not [f for f, src in hips.items() if "0x7ffffff0" in src.lower()]
    rsrc = [(f, line.strip()) for f, src in hips.items() for line in src.splitlines() if "__builtin_amdgcn_make_buffer_rsrc" in line]
    assert len(rsrc) == 1 and rsrc[0][0] == "gemm.hip" and "slab_rs" in rsrc[0][1], rsrc
    header = open(os.path.join(csrc, "gfx950.h")).read()
    assert '#include "gfx950.h"' in open(os.path.join(csrc, "common.h")).read()
    for name in PRIMITIVES:
        definition = re.compile(r"(?:__device__ __forceinline__ \w+|#define|constexpr unsigned) %s\b" % name)
        assert len(definition.findall(header)) == 1, name
        assert not [f for f, src in hips.items() if definition.search(src)], name
