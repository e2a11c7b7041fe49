"""The per-block C entries of SHARP_unlimited, called directly (sharp_amd/csrc/unlimited.hip): sharp_unlimited_block_dev, ..._dev64 and
..._view_dev are not reached through the Python layer (device.unlimited_block_dev always takes the viewk entries), and all five share one
body.  One small seeded block on the SHARP_small path: the entries agree table for table, the thread's view arm is taken once, and every
refusal keeps its text."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED, RS = 20261003, 2103
N, M, K, P, G = 600, 200, 3, 10, 4
CAP = 64


def _table(entry, x, proj, *tail, cap=CAP, counts=True, viE=None):
    """One call of a per-block entry: (rc, labels, means of the first G rows, sizes, viE).  tail: what the entry takes between rN_seed and
    pred (the flag of the view entries) and behind counts (view_dim, view_seed) -- viE, where the entry has one, goes last."""
    from sharp_amd._lib import f64, i32, i64

    pred = np.zeros(x.shape[0], np.int32)
    means = np.full((CAP, P), np.nan)
    cnt = np.zeros(CAP, np.int64)
    g = C.c_int(-1)
    pre, post = tail[:1], tail[1:]
    args = [x.data_ptr(), M, x.shape[0], x.stride(0), P, proj.handle, K, RS, *pre, i32(pred), C.byref(g), f64(means), cap,
            i64(cnt) if counts else None, *post]
    if pre:
        args.append(f64(viE))
    rc = entry(*args)
    return rc, pred, means[:max(g.value, 0)].copy(), cnt[:max(g.value, 0)].copy(), viE


@pytest.fixture(scope="module")
def env():
    import torch

    import sharp_amd
    from sharp_amd import device as dev

    sharp_amd.init(0)
    lib = sharp_amd.lib()
    x = torch.empty((N, M), dtype=torch.float32, device="cuda")
    dev.synth_fill(x, SEED, 0, G, 40)
    x64 = x.double().contiguous()
    torch.cuda.synchronize()
    proj = sharp_amd.Projector(M, P, [50 + RS + k for k in range(1, K + 1)])
    rc, pred, means, cnt, _ = _table(lib.sharp_unlimited_block_dev, x, proj)        # the reference table: computed once, never written to
    assert rc == 0, lib.sharp_last_error()
    assert len(cnt) >= 2 and cnt.sum() == N and pred.min() == 1 and pred.max() == len(cnt)
    for a in (pred, means, cnt):
        a.setflags(write=False)
    yield lib, x, x64, proj, (pred, means, cnt)
    proj.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


def test_fp32_entries_return_one_table(env):
    lib, x, _, proj, ref = env
    rc, *view = _table(lib.sharp_unlimited_block_view_dev, x, proj, 1)
    assert rc == 0, lib.sharp_last_error()
    rc, *viewk = _table(lib.sharp_unlimited_block_viewk_dev, x, proj, 1, 0, 0.0)
    assert rc == 0, lib.sharp_last_error()
    assert _same(view, ref) and _same(viewk, ref)


def test_fp64_entries_return_one_table(env):
    # (fp64 against fp64 only: tests/test_x_storage_gpu.py:57-65 asserts fp32 = fp64 storage for the host entry on un-logged counts of the
    # large path, not for these entries on a logged block)
    lib, _, x64, proj, ref = env
    rc, *d64 = _table(lib.sharp_unlimited_block_dev64, x64, proj)
    assert rc == 0, lib.sharp_last_error()
    rc, *k64 = _table(lib.sharp_unlimited_block_viewk_dev64, x64, proj, 1, 0, 0.0)
    assert rc == 0, lib.sharp_last_error()
    assert _same(k64, d64)
    assert len(d64[2]) >= 1 and d64[2].sum() == N


def test_view_arm_is_taken_by_one_call(env):
    lib, x, _, proj, ref = env
    assert lib.sharp_unlimited_view_dim(4) == 0
    rc, *armed, v4 = _table(lib.sharp_unlimited_block_view_dev, x, proj, 1, viE=np.full(N * P, np.nan))
    assert rc == 0, lib.sharp_last_error()
    assert np.isfinite(v4[:N * 4]).all() and np.isnan(v4[N * 4:]).all()            # four columns per cell
    rc, *spent, vp = _table(lib.sharp_unlimited_block_view_dev, x, proj, 1, viE=np.full(N * P, np.nan))
    assert rc == 0, lib.sharp_last_error()
    assert np.isfinite(vp).all()                                                    # the arm is spent: E1 itself, p columns
    assert _same(armed, ref) and _same(spent, ref)
    # the same two through the entry that names its view: the arm's seed is the next of the run's sequence, 50 + rN.seed + K + 1
    rc, *_, k4 = _table(lib.sharp_unlimited_block_viewk_dev, x, proj, 1, 4, float(50 + RS + K + 1), viE=np.full(N * P, np.nan))
    assert rc == 0, lib.sharp_last_error()
    rc, *_, kp = _table(lib.sharp_unlimited_block_viewk_dev, x, proj, 1, 0, 0.0, viE=np.full(N * P, np.nan))
    assert rc == 0, lib.sharp_last_error()
    assert k4.tobytes() == v4.tobytes() and kp.tobytes() == vp.tobytes()
    assert np.abs(v4[:N * 4]).max() > 0 and np.abs(vp).max() > 0


def test_refusals_keep_their_text(env):
    lib, x, x64, proj, ref = env
    assert len(ref[2]) > 1
    entries = [(lib.sharp_unlimited_block_dev, x, (), "sharp_unlimited_block_dev"),
               (lib.sharp_unlimited_block_dev64, x64, (), "sharp_unlimited_block_dev64"),
               (lib.sharp_unlimited_block_view_dev, x, (1,), "sharp_unlimited_block_view_dev"),
               (lib.sharp_unlimited_block_viewk_dev, x, (1, 0, 0.0), "sharp_unlimited_block_view_dev"),
               (lib.sharp_unlimited_block_viewk_dev64, x64, (1, 0, 0.0), "sharp_unlimited_block_view_dev")]
    for entry, blk, tail, name in entries:
        rc = _table(entry, blk, proj, *tail, cap=1)[0]                              # more clusters than rows
        assert rc != 0 and lib.sharp_last_error().decode() == name + ": centroid buffer too small", name
        rc = _table(entry, blk, proj, *tail, counts=False)[0]
        assert rc != 0 and lib.sharp_last_error().decode() == name + ": null output", name
    for entry, blk, name in ((lib.sharp_unlimited_block_viewk_dev, x, "sharp_unlimited_block_viewk_dev"),
                             (lib.sharp_unlimited_block_viewk_dev64, x64, "sharp_unlimited_block_viewk_dev64")):
        text = name + ": view_dim must lie in 0 .. 4096 and view_seed must be an integer (the seed of the run's z0)"
        rc = _table(entry, blk, proj, 1, 5000, 7.0, viE=np.zeros(N * P))[0]
        assert rc != 0 and lib.sharp_last_error().decode() == text, name
        rc = _table(entry, blk, proj, 1, 4, 7.5, viE=np.zeros(N * P))[0]
        assert rc != 0 and lib.sharp_last_error().decode() == text, name
    rc, *again = _table(lib.sharp_unlimited_block_dev, x, proj)                     # and a refused call leaves nothing behind
    assert rc == 0 and _same(again, ref)


def test_blocks_in_one_call_return_the_blocks_tables(env):
    """Two such blocks through sharp_unlimited_blocks_dev: per block the table of sharp_unlimited_block_dev -- labels, sizes and means
    exactly, as tests/test_configs_gpu.py:451 asserts for large blocks (np.array_equal on all three); blocks of this size go block after
    block through the same call, so nothing weaker holds here."""
    import torch

    from sharp_amd import device as dev
    from sharp_amd._lib import f64, i32, i64

    lib, x, _, proj, ref = env
    y = torch.empty((N + 37, M), dtype=torch.float32, device="cuda")
    dev.synth_fill(y, SEED, 40000, G, 40)
    rc, *ty = _table(lib.sharp_unlimited_block_dev, y, proj)
    assert rc == 0, lib.sharp_last_error()
    many = dev.unlimited_blocks_dev([x, y], P, proj.handle, K, RS, cap_rows=CAP)
    assert len(many) == 2
    for got, one in zip(many, (ref, ty)):
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[2], one[2]) and np.array_equal(got[1], one[1])
    # its own refusals: the running row offset against cap_rows, a null table
    ptrs = (C.c_void_p * 2)(x.data_ptr(), y.data_ptr())
    ncb, ldb = np.array([N, N + 37], np.int64), np.array([M, M], np.int64)
    pred, ncl, means, cnt = np.zeros(2 * N + 37, np.int32), np.zeros(2, np.int32), np.zeros((2 * CAP, P)), np.zeros(2 * CAP, np.int64)
    rc = lib.sharp_unlimited_blocks_dev(ptrs, None, i64(ncb), i64(ldb), 2, M, P, proj.handle, K, RS, i32(pred), i32(ncl), f64(means), len(ref[2]), i64(cnt))
    assert rc != 0 and lib.sharp_last_error().decode() == "sharp_unlimited_blocks_dev: centroid buffer too small"
    rc = lib.sharp_unlimited_blocks_dev(ptrs, None, i64(ncb), i64(ldb), 2, M, P, proj.handle, K, RS, i32(pred), i32(ncl), f64(means), 2 * CAP, None)
    assert rc != 0 and lib.sharp_last_error().decode() == "sharp_unlimited_blocks_dev: null argument"
