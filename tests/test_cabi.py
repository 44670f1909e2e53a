"""The C-ABI shared library: loads, exports exactly what include/gf2bv_hip.h declares, validates
arguments like the reference boundary, and refuses to solve without a GPU.  No compute calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from gf2bv_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gf2bv_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gf2bv_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_all_exported():
    decl = declared_symbols()
    assert decl == sorted(hip.EXPORTS)
    L = hip.lib()
    for name in decl:
        assert hasattr(L, name), name
    dyn = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gf2bv_[a-z_0-9]+)", dyn))
    assert set(decl) <= exported


def test_no_torch_types_in_abi():
    text = open(HEADER).read()
    assert "torch" not in text.lower().replace("no torch", "") and "at::" not in text and "hipStream_t" not in text.replace("hipStream_t or NULL", "")


def test_argument_validation_precedes_device_use():
    L = hip.lib()
    h = ctypes.c_void_p()
    aug = np.zeros((4, 1), dtype=np.uint64)
    assert L.gf2bv_solve_words(aug.ctypes.data, 4, 0, 1, 0, 0, ctypes.byref(h)) == 1          # cols <= 0
    assert b"columns must be positive" in L.gf2bv_last_error()
    assert L.gf2bv_solve_words(aug.ctypes.data, 4, 4, 1, 7, 0, ctypes.byref(h)) == 1          # bad mode
    assert b"Invalid mode" in L.gf2bv_last_error()
    assert L.gf2bv_solve_words(aug.ctypes.data, 3, 4, 1, 0, 0, ctypes.byref(h)) == 1          # rows < cols
    assert b"greater than or equal" in L.gf2bv_last_error()
    assert L.gf2bv_solve_words(aug.ctypes.data, 80, 70, 1, 0, 0, ctypes.byref(h)) == 1        # stride too small
    with pytest.raises(ValueError):
        hip.solve_words(aug, 3, 4)
    assert L.gf2bv_version() >= 100


def test_single_entries_check_arguments_before_device_use():
    """gf2bv_solve_{words,digits,device} refuse the bad arguments their rhs and factor siblings refuse: GF2BV_ERR_ARG (1) with the
    same message, on a machine without a GPU too (GF2BV_ERR_NODEVICE would be 2).  So does the matrix check of gf2bv_slab_open."""
    L = hip.lib()
    rows, cols = 130, 100
    aug = np.zeros((rows + 1, 2), dtype=np.uint64)
    off = np.zeros(rows + 1, dtype=np.int64)
    dig = np.zeros(4, dtype=np.uint32)
    A, O, D = aug.ctypes.data, off.ctypes.data, dig.ctypes.data
    h = ctypes.c_void_p(0)
    H = ctypes.byref(h)

    def err(rc, what):
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()

    err(L.gf2bv_solve_words(A, rows, cols, 2, 0, 0, None), "null")
    err(L.gf2bv_solve_words(None, rows, cols, 2, 0, 0, H), "null")
    err(L.gf2bv_solve_words(A, rows, cols, 1, 0, 0, H), "stride")
    err(L.gf2bv_solve_words(A, 99, cols, 2, 0, 0, H), "greater than or equal")
    err(L.gf2bv_solve_words(A, rows, cols, 2, 3, 0, H), "Invalid mode")
    err(L.gf2bv_solve_words(A, rows, 0, 2, 0, 0, H), "columns must be positive")
    err(L.gf2bv_solve_digits(D, None, 30, rows, cols, 0, 0, H), "null")
    err(L.gf2bv_solve_digits(D, O, 0, rows, cols, 0, 0, H), "bits_per_digit")
    err(L.gf2bv_solve_digits(D, O, 33, rows, cols, 0, 0, H), "bits_per_digit")
    err(L.gf2bv_solve_digits(D, O, 30, rows, cols, 0, 0, None), "null")
    err(L.gf2bv_solve_digits(D, O, 30, 99, cols, 0, 0, H), "greater than or equal")
    err(L.gf2bv_solve_digits(D, O, 30, rows, cols, 3, 0, H), "Invalid mode")
    err(L.gf2bv_solve_digits(D, O, 30, rows, 0, 0, 0, H), "columns must be positive")
    bad_off = off.copy()
    bad_off[0] = 1
    err(L.gf2bv_solve_digits(D, bad_off.ctypes.data, 30, rows, cols, 0, 0, H), "start at 0")
    bad_off = off.copy()
    bad_off[5:] = 3
    bad_off[9] = 2
    err(L.gf2bv_solve_digits(D, bad_off.ctypes.data, 30, rows, cols, 0, 0, H), "must not decrease")
    some_off = np.arange(rows + 1, dtype=np.int64)
    err(L.gf2bv_solve_digits(None, some_off.ctypes.data, 30, rows, cols, 0, 0, H), "null")
    err(L.gf2bv_solve_device(None, rows, cols, 2, 0, 0, None, 0, H), "null")
    err(L.gf2bv_solve_device(A, rows, cols, 2, 0, 0, None, 0, None), "null")
    err(L.gf2bv_solve_device(A, rows, cols, 3, 0, 0, None, 0, H), "stride")
    err(L.gf2bv_solve_device(A, rows, cols, 1, 0, 0, None, 0, H), "stride")
    err(L.gf2bv_solve_device(A + 8, rows, cols, 2, 0, 0, None, 0, H), "16-byte alignment")
    err(L.gf2bv_solve_device(A, 99, cols, 2, 0, 0, None, 0, H), "greater than or equal")
    err(L.gf2bv_solve_device(A, rows, cols, 2, 3, 0, None, 0, H), "Invalid mode")
    err(L.gf2bv_solve_device(A, rows, 0, 2, 0, 0, None, 0, H), "columns must be positive")
    assert not h.value                                          # nothing was made
    work = np.zeros(L.gf2bv_slab_work_words(rows, cols) + 2, dtype=np.uint64)
    W, WW = work.ctypes.data, L.gf2bv_slab_work_words(rows, cols)
    W = W + (-W % 16)                                          # (a 16-byte aligned working matrix)
    err(L.gf2bv_slab_open(A, rows, cols, 3, W, WW, 1, 0, 0, H), "stride")
    err(L.gf2bv_slab_open(A + 8, rows, cols, 2, W, WW, 1, 0, 0, H), "16-byte alignment")
    err(L.gf2bv_slab_open(A, rows, cols, 2, W + 8, WW, 1, 0, 0, H), "16-byte alignment")
    err(L.gf2bv_slab_open(A, 99, cols, 2, W, WW, 1, 0, 0, H), "greater than or equal")
    err(L.gf2bv_slab_open(A, rows, cols, 2, W, WW - 1, 1, 0, 0, H), "too small")
    assert not h.value
    # gf2bv_quad_plan_device: the space and the outputs are checked like gf2bv_quad_plan's, in front of the device
    r, re, m, fw = (ctypes.c_int64() for _ in range(4))
    outs = (ctypes.byref(r), ctypes.byref(re), ctypes.byref(m), ctypes.byref(fw), None, 0)
    err(L.gf2bv_quad_plan_device(None, A, 0, 2, 10, 0, *outs), "null")
    err(L.gf2bv_quad_plan_device(A, None, 3, 2, 10, 0, *outs), "null")
    err(L.gf2bv_quad_plan_device(A, A, -1, 2, 10, 0, *outs), "dimension")
    err(L.gf2bv_quad_plan_device(A, A, 0, 2, 0, 0, *outs), "n_lin")
    err(L.gf2bv_quad_plan_device(A, A, 0, 1, 12, 0, *outs), "words does not cover")
    err(L.gf2bv_quad_plan_device(A, A, 0, 2, 10, 0, None, *outs[1:]), "null")
    err(L.gf2bv_quad_plan_device(A, A, 0, 2, 10, 0, *outs[:3], None, None, 0), "null")


def test_batch_entries_check_arguments_before_device_use():
    """gf2bv_solve_batch_{device,digits,digits_multi} check in the single entries' order -- out, shape, form, then the device --
    and fail with GF2BV_ERR_ARG (1) and a specific message, on a machine without a GPU too; every out[s] is null afterwards."""
    L = hip.lib()
    nsys, rows, cols = 3, 130, 100
    aug = np.zeros((nsys * rows + 1, 2), dtype=np.uint64)
    A, SS = aug.ctypes.data, rows * 2
    off = np.zeros(nsys * rows + 1, dtype=np.int64)
    dig = np.zeros(4, dtype=np.uint32)
    O, D = off.ctypes.data, dig.ctypes.data
    devices = (ctypes.c_int * 1)(0)
    out = (ctypes.c_void_p * nsys)()

    def err(call, what, cleared=True):
        for s in range(nsys):
            out[s] = 0x1000 + s                                 # never a handle: cleared before anything can free it
        rc = call()
        assert rc == 1, (rc, L.gf2bv_last_error())
        assert what.encode() in L.gf2bv_last_error(), L.gf2bv_last_error()
        if cleared:
            assert not any(out[s] for s in range(nsys)), list(out)

    def dev(d_aug=A, sys_stride=SS, r=rows, stride=2, mode=0, o=out):
        return lambda: L.gf2bv_solve_batch_device(d_aug, nsys, sys_stride, r, cols, stride, mode, 0, None, 0, o)

    err(dev(o=None), "null", cleared=False)
    err(dev(d_aug=None), "null")
    err(dev(mode=3), "Invalid mode")
    err(dev(r=99), "greater than or equal")
    err(dev(stride=3, sys_stride=rows * 4), "stride")
    err(dev(stride=1), "stride")
    err(dev(d_aug=A + 8), "16-byte alignment")
    err(dev(sys_stride=SS + 1), "sys_stride_words")
    err(dev(sys_stride=SS - 2), "sys_stride_words")

    decreasing = np.arange(nsys * rows + 1, dtype=np.int64) + 7   # (absolute: a share of a larger batch need not start at 0)
    decreasing[200] = 3
    some = np.arange(nsys * rows + 1, dtype=np.int64) + 7

    def digs(digits=D, offsets=O, bpd=30, r=rows, mode=0, o=out):
        return [lambda: L.gf2bv_solve_batch_digits(digits, offsets, bpd, nsys, r, cols, mode, 0, o),
                lambda: L.gf2bv_solve_batch_digits_multi(digits, offsets, bpd, nsys, r, cols, mode, devices, 1, o)]

    for call in digs(o=None):
        err(call, "null", cleared=False)
    checks = [(digs(offsets=None), "null"), (digs(mode=3), "Invalid mode"), (digs(r=99), "greater than or equal"),
              (digs(bpd=0), "bits_per_digit"), (digs(bpd=33), "bits_per_digit"),
              (digs(offsets=decreasing.ctypes.data), "must not decrease"),
              (digs(digits=None, offsets=some.ctypes.data), "null")]
    for calls, what in checks:
        for call in calls:
            err(call, what)
    err(lambda: L.gf2bv_solve_batch_digits_multi(D, O, 30, nsys, rows, cols, 3, None, 0, out), "Invalid mode")
    err(lambda: L.gf2bv_solve_batch_digits_multi(D, O, 30, nsys, rows, cols, 0, None, 0, out), "null")


def test_no_cpu_fallback():
    if hip.device_count() > 0:
        pytest.skip("a GPU is present")
    aug = np.zeros((4, 1), dtype=np.uint64)
    with pytest.raises(hip.HipError, match="no HIP device"):
        hip.solve_words(aug, 4, 4)
    with pytest.raises(hip.HipError):
        hip.DeviceBuffer(1024)


def test_space_combine_host_helper():
    L = hip.lib()
    origin = np.array([0b0001, 7], dtype=np.uint64)
    basis = np.array([[0b0101, 0], [0b1000, 1], [0, 1 << 63]], dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint64)
    sel = np.array([0b101], dtype=np.uint64)
    L.gf2bv_space_combine(origin.ctypes.data, basis.ctypes.data, 3, 2, sel.ctypes.data, 1, out.ctypes.data)
    assert list(out) == [0b0001 ^ 0b0101, 7 ^ (1 << 63)]


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under gf2bv_amd/ may reference it, and outside tests/ only
    __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it."""
    pkg = os.path.join(ROOT, "gf2bv_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle" not in src.lower() or f == "__none__", os.path.join(dirpath, f)
    for sub in ("tools", "examples"):
        for f in os.listdir(os.path.join(ROOT, sub)):
            if f.endswith((".py", ".hip")):
                src = open(os.path.join(ROOT, sub, f), errors="replace").read()
                assert "import gf2_oracle" not in src and "from oracle" not in src, os.path.join(sub, f)
    bench = open(os.path.join(ROOT, "bench.py")).read()
    # every import of the oracle sits inside a cpu_baseline* function (the synthetic headline sample; the list-of-int systems
    # of the c3 / c5 legs): timed beside the GPU numbers and used as their checker, never as the thing measured
    parts = bench.split("from oracle import")
    assert 2 <= len(parts) <= 3
    for head in (("from oracle import".join(parts[:k])) for k in range(1, len(parts))):
        assert head.rsplit("\ndef ", 1)[-1].startswith("cpu_baseline"), head.rsplit("\ndef ", 1)[-1][:40]
    assert "oracle" not in bench.split("def timed_single")[1].split("def run_single")[0]      # the timed region itself


def test_round5_entry_points_without_a_device():
    """The planning / pool / staging entry points of round 5 on a box without a GPU: the gang planner is a pure function, the pool
    calls report "no device" instead of touching one, pinned staging is refused (the binding then falls back to malloc), and the
    optional true-M4RI timing says that there is no libm4ri here."""
    import ctypes
    L = hip.lib()
    # 64 systems of 32768^2 with a whole MI355X free: two gangs of 32 (one per host thread, multiples of 8 for a system per XCD)
    assert L.gf2bv_plan_gang(64, 32768, 32768, 280 * 10 ** 9) == 32
    assert L.gf2bv_plan_gang(512, 32768, 32768, 200 * 10 ** 9) == 32
    assert L.gf2bv_plan_gang(5, 2048, 2048, 10 ** 9) >= 1 and L.gf2bv_plan_gang(0, 1, 1, 1) == 0
    assert L.gf2bv_plan_gang(64, 32768, 32768, 2 * 10 ** 9) <= 6          # (little memory left: the gang shrinks to what fits)
    if hip.device_count() == 0:
        assert L.gf2bv_pool_trim(0) == -1
        p = ctypes.c_void_p()
        assert L.gf2bv_host_alloc(1 << 20, ctypes.byref(p)) == 2 and not p.value
    assert L.gf2bv_pool_idle_bytes(-1) == -1
    out = (ctypes.c_int64 * 3)(7, 7, 7)
    assert L.gf2bv_pool_in_use(-1, out) == -1 and L.gf2bv_pool_in_use(0, None) == -1 and list(out) == [7, 7, 7]
    if hip.device_count() == 0:                    # (nothing has been handed out where there is no device)
        assert L.gf2bv_pool_in_use(0, out) == 0 and list(out) == [0, 0, 0]
        assert hip.pool_in_use(0) == {"buffers": 0, "streams": 0, "events": 0}
    L.gf2bv_host_free(None)
    assert L.gf2bv_host_pool_trim() >= 0
    from oracle import gf2_oracle as O
    r = O.m4ri_time(256)
    assert r["found"] in (True, False) and (r["found"] or "libm4ri" in r["why"])
