"""The pixel kernels' table and the selection of an entry, without a GPU.

The library names every decode_kernel<S, F, V> / decode_kernel_lat<S, F, V> it
instantiates once, in one table keyed (latency, S, F, V); a launch checks its
shape, computes the key and looks it up.  Checked here: the table against the
function symbols of the built library's gfx950 code objects, and
hjd_debug_kernel_key over the whole cross product of its arguments against a
second statement of the rules (model() below, written from the rules, with
the kernels' bit values as plain numbers)."""
import ctypes
import glob
import itertools
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools", "check"))
import d16_order  # noqa: E402  (the code-object extraction's llvm-objdump and architecture)

LIB = os.path.join(REPO, "ocljpegdecoder_amd", "lib", "libhjd.so")
LAT_TASKS = 1024
STAGES = (4, 8, 16, 20, 24, 64, 80, 256)
# the sweep: every argument of hjd_debug_kernel_key, legal and illegal values
AXES = dict(sampling=range(8), input_format=(0, 1, 2), out_format=range(8), scale=(1, 2, 3, 4, 8, 16), roi=(0, 1),
            variant=range(5), stages=(0,) + STAGES + (5,), kernel_mode=(0, 1, 2, 3),
            tasks=(1, LAT_TASKS, LAT_TASKS + 1, 2 ** 31), grid_blocks=(0, 7), d16=(0, 1))


def pack(latency, s, f, v):
    """One integer per key (V has 16 bits)."""
    return (latency << 24) | (s << 20) | (f << 16) | v


@pytest.fixture(scope="module")
def table(hjd):
    lib = hjd._lib.load()
    n = lib.hjd_debug_kernel_table(None, 0)
    keys = np.zeros((n, 4), dtype=np.int32)
    assert lib.hjd_debug_kernel_table(keys.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n) == n
    return keys


def test_table_has_331_distinct_keys(table):
    assert len(table) == 331
    assert len({tuple(k) for k in table.tolist()}) == 331
    lat = table[:, 0] == 1
    assert (int(lat.sum()), int((~lat).sum())) == (60, 271)
    assert set(table[:, 0].tolist()) == {0, 1} and set(table[:, 1].tolist()) == set(range(6))


@pytest.mark.skipif(not os.path.exists(d16_order.LLVM_OBJDUMP), reason="llvm-objdump is not installed")
def test_table_is_the_librarys_kernel_set(table):
    """Every decode_kernel / decode_kernel_lat function of the built code objects is in the table, and the reverse."""
    tmp = tempfile.mkdtemp(prefix="hjd_ktable_")
    try:
        dst = os.path.join(tmp, os.path.basename(LIB))
        shutil.copy(LIB, dst)
        subprocess.run([d16_order.LLVM_OBJDUMP, "--offloading", dst], cwd=tmp, check=True, capture_output=True)
        objs = sorted(glob.glob(os.path.join(tmp, f"*{d16_order.ARCH}*")))
        assert objs
        syms = "\n".join(subprocess.run([d16_order.LLVM_OBJDUMP, "-t", "-C", co], check=True, capture_output=True,
                                        text=True).stdout for co in objs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    built = {(int(m.group(1) is not None), int(m.group(2)), int(m.group(3)), int(m.group(4)))
             for m in re.finditer(r"hjd::decode_kernel(_lat)?<(\d+), (\d+), (\d+)>\(", syms)}
    listed = {tuple(k) for k in table.tolist()}
    assert built - listed == set(), "instantiated, not in the table"
    assert listed - built == set(), "in the table, not in the code objects"


def model(a):
    """(ok, packed key) for arrays of the arguments: the rules of DESIGN.md s3.8, restated."""
    samp, fmt, out, scale, roi, var, stg, mode, tasks, grid, d16 = (a[k] for k in AXES)
    s_index = np.select([samp == 0, samp == 1, samp == 3, samp == 4, samp == 5, samp == 6], [0, 1, 2, 3, 4, 5], -1)
    lg = np.select([scale == 1, scale == 2, scale == 4, scale == 8], [0, 1, 2, 3], -1)
    out_bits = np.select([out == 0, out == 1, out == 2, out == 3, out == 5, out == 6],
                         [0, 32, 512, 1024, 1024 | 1 << 14, 1024 | 1 << 15], -1)
    is_float = (out == 5) | (out == 6)
    whole = (lg == 0) & (roi == 0)                     # whole frames at full size
    staged = stg != 0
    ok = (s_index >= 0) & (fmt <= 1) & (out_bits >= 0) & (lg >= 0) & (var <= 3) & (mode <= 2)
    ok &= (stg == 0) | np.isin(stg, STAGES)
    ok &= (fmt == 0) | (whole & ~is_float)             # int32 input: whole full-size frames in a byte format
    ok &= (lg <= 0) | np.isin(samp, (0, 1, 4))         # scaled: 4:4:4, 4:2:0 and gray
    ok &= (mode != 2) | whole                          # no latency kernel scaled or with a ROI
    ok &= ~staged | ((fmt == 0) & (out == 0) & (s_index <= 1) & whole & (var == 0))
    # 1: the latency kernel, on request or for a small AUTO launch with the default grid
    latency = ~staged & whole & ((mode == 2) | ((mode == 0) & (grid == 0) & (tasks <= LAT_TASKS)))
    ok &= ~latency | (tasks <= 2 ** 31 - 1)
    # 2: the latency kernels ignore variant bits 0-1.  4: a persistent launch refuses them with a
    # non-BGRX format; scaled, ROI and float shapes refuse them whatever the kernel
    ok &= (var == 0) | (whole & ~is_float & ((out == 0) | latency))
    # 3: the d16 twin
    twin = (d16 != 0) & (samp == 0) & (fmt == 0) & ~latency & whole & ((var & 2) == 0)
    v = np.where(latency, out_bits, out_bits | (lg << 11) | (roi << 13) | var | stg | np.where(twin, 128, 0))
    return ok, pack(latency.astype(np.int64), s_index, fmt, v)


def test_every_shape_selects_what_the_rules_say(hjd, table):
    lib = hjd._lib.load()
    listed = set(pack(*table.T.astype(np.int64)).tolist())
    assert len(listed) == 331
    fn = lib.hjd_debug_kernel_key
    saved = fn.argtypes
    fn.argtypes = saved[:-1] + [ctypes.c_void_p]       # keys land in the chunk's array at their point's row
    names = list(AXES)
    inner = [np.asarray(AXES[k], dtype=np.int64) for k in names[1:]]
    grids = np.meshgrid(*inner, indexing="ij")         # itertools.product's order
    n = grids[0].size
    reached = set()
    check = hjd._lib.check
    check(lib.hjd_debug_set_tuning(b"HJD_LAT_TASKS", str(LAT_TASKS).encode()), "hjd_debug_set_tuning")
    try:
        for samp in AXES["sampling"]:
            keys = np.full((n, 4), -1, dtype=np.int32)
            base = keys.ctypes.data
            rcs = np.array([fn(samp, *p, base + 16 * i)
                            for i, p in enumerate(itertools.product(*[AXES[k] for k in names[1:]]))], dtype=np.int64)
            args = dict(zip(names[1:], (g.ravel() for g in grids)), sampling=np.full(n, samp, dtype=np.int64))
            ok, want = model(args)
            assert set(np.unique(rcs).tolist()) <= {0, -1}
            got_ok = rcs == 0
            bad = np.flatnonzero(got_ok != ok)
            assert bad.size == 0, ("status", {k: int(args[k][bad[0]]) for k in names}, int(rcs[bad[0]]))
            got = pack(*keys[got_ok].T.astype(np.int64))
            bad = np.flatnonzero(got != want[ok])
            assert bad.size == 0, ("key", {k: int(args[k][ok][bad[0]]) for k in names}, keys[got_ok][bad[0]].tolist())
            reached |= set(np.unique(got).tolist())
    finally:
        fn.argtypes = saved
        check(lib.hjd_debug_set_tuning(b"HJD_LAT_TASKS", None), "hjd_debug_set_tuning")
    assert reached - listed == set(), "a selected key is not in the table"
    assert listed - reached == set(), "a table entry no shape selects"
