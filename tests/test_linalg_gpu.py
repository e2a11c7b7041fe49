"""The fp64 MFMA GEMM kernels and the row preparation in front of them (sharp_amd/csrc/linalg.hip) against plain numpy restatements
(tests/_linalg_ref.py, pinned by tests/test_linalg_cpu.py), directly: ragged M / N / K, both GEMM kernels, the three epilogues, the
symmetric (mirrored) form, whole batches with unequal tasks, sliced launches, padded outputs, the per-tile row minima, and the three
modes and three code paths of the row preparation with the zero padding of Ct.

The batch tests go through sharp_gemm_tn_f64_batch / sharp_row_prep_batch (include/sharp_hip.h): ONE descriptor array, one
gemm_tn_f64_batched / row_prep_batched call, operands padded as the production callers pad them, and every output pre-filled with a NaN
of a fixed bit pattern, so that a test sees what was written and what was not.

Where a result can be exact it is compared bit for bit: integer operands (every partial sum an integer below 2^53 in any order),
operands in eighths (products in 64ths: the clamps, 1 - v and v * v are exact), copies, zero padding, and the row minima, which are a
selection among values the same call stored.  Continuous products are held to the textbook bound of a K-term dot product
(_linalg_ref.gemm_bound).

Tolerance of the row preparation, derived (first order in p u, u = 2^-53; fp64 operations in ANY summation order, no cancellation
relied upon).  Per row let A = |mean| + max |x - mean| >= max |x|, kappa = A / sd the row's conditioning, zmax = max |x - mean| / sd,
f = sqrt(p / (p - 1)), all taken from the reference.
  mean:        a sum of p terms and a division: |d mean| <= p u A.
  c = x - mean: |dc| <= p u A + u |c|                                                        [mode 1's Cr: (p + 1) u A]
  ss = sum c^2: |d ss| <= 2 sum |c| |dc| + (p + 1) u ss with sum |c| <= sqrt(p ss) and sqrt(ss) = sd sqrt(p - 1), so relative
               2 f p u kappa + (p + 3) u; sd = sqrt(ss / (p - 1)) takes half of it and two more roundings:
               rho = f p u kappa + (p / 2 + 4) u.
  z = c / sd:  |dz| <= |dc| / sd + |z| (rho + u) <= ez = p u kappa + zmax (rho + 2 u).
  mean2:       the mean of the computed z: within ez of the mean of the true z (0), plus its own summation p u mean |z| <= p u.
  c2 = z - mean2: |d c2| <= e2 = 2 ez + (p + zmax) u.
  ||c2||:      true value sqrt(p - 1); as for ss, relative rho_n = f e2 + (p / 2 + 2) u.
  Cr = c2 / ||c2||, |Cr| <= 1:  |d Cr| <= e2 / sqrt(p - 1) + rho_n + u, and one more u for the reference rounded to fp64.
  mode 1's nrm = sqrt(sum c^2): sqrt(p) p u A + (p / 2 + 3) u nrm, and one more u nrm likewise.
At the shapes below that is 1e-14 (p = 3) to 7e-12 (p = 1030) of a unit vector's entries; tests/test_linalg_cpu.py shows that a
sequential fp64 restatement stays within it against the longdouble reference (measured there: 1.6e-16 at most), so the bound is
measured against the reference and not against the kernels."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _linalg_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd.lib()


def _gemm(lib, At, Bt, epilogue=0, symmetric=0, fast=0):
    K, M = At.shape
    N = M if symmetric else Bt.shape[1]
    Cm = np.full((M, N), np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.sharp_gemm_tn_f64(dp(At), dp(At if symmetric else Bt), dp(Cm), M, N, K, epilogue, symmetric, fast)
    assert rc == 0, lib.sharp_last_error()
    return Cm


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (63, 65, 17), (64, 64, 16), (130, 127, 391), (257, 40, 5), (300, 513, 33), (128, 128, 474)])
def test_plain_product(lib, fast, M, N, K):
    rng = np.random.default_rng(M * 1000 + N + K)
    At, Bt = rng.standard_normal((K, M)), rng.standard_normal((K, N))
    got = _gemm(lib, At, Bt, fast=fast)
    ref = At.T @ Bt
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13 * K * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("n,K", [(5, 3), (129, 100), (200, 391), (385, 16)])
def test_symmetric_correlation_epilogues(lib, fast, n, K):
    rng = np.random.default_rng(n + K)
    U = rng.standard_normal((K, n))
    U -= U.mean(0)
    U /= np.linalg.norm(U, axis=0)                      # unit centred columns: U^T U is a correlation matrix
    cor = np.clip(U.T @ U, -1, 1)
    d = _gemm(lib, U, U, epilogue=1, symmetric=1, fast=fast)
    ref = 1 - cor
    np.fill_diagonal(ref, 0.0)
    np.testing.assert_allclose(d, ref, rtol=0, atol=1e-13 * K)
    assert np.array_equal(d, d.T) and np.all(np.diag(d) == 0.0)        # mirrored, exact diagonal
    sres = _gemm(lib, U, U, epilogue=2, symmetric=1, fast=fast)
    ref2 = cor.copy()
    np.fill_diagonal(ref2, 1.0)
    np.testing.assert_allclose(sres, ref2, rtol=0, atol=1e-13 * K)
    assert np.array_equal(sres, sres.T) and np.all(np.diag(sres) == 1.0) and sres.max() <= 1.0


# ---- batches, padding, minima: through the batch test entries -----------------------------------------------------------------------
def _written(a):
    """which elements of a returned buffer no longer hold the sentinel the entry filled it with"""
    return np.ascontiguousarray(a).view(np.uint64) != R.SENTINEL_BITS


def _gemm_batch_raw(lib, M, N, K, At, Bt, *, epilogue=0, symmetric=0, fast=0, nn_square=0, want_nn=0, polite=0, ldc_pad=0):
    """sharp_gemm_tn_f64_batch on concatenated operands -> the concatenated C and nn buffers, whole"""
    M, N, K = (np.ascontiguousarray(a, np.int32) for a in (M, N, K))
    ldc = R.rup(N.astype(np.int64), 128) if ldc_pad else N.astype(np.int64)
    Cbuf = np.zeros(int((M * ldc).sum()))
    nnbuf = np.zeros(int((ldc // 128 * ldc).sum())) if want_nn else None
    At = np.ascontiguousarray(At, np.float64)
    Bt = None if Bt is None else np.ascontiguousarray(Bt, np.float64)
    assert At.size == int((K.astype(np.int64) * M).sum()) and (Bt is None or Bt.size == int((K.astype(np.int64) * N).sum()))
    rc = lib.sharp_gemm_tn_f64_batch(len(M), M.ctypes.data, N.ctypes.data, K.ctypes.data, At.ctypes.data, None if Bt is None else Bt.ctypes.data,
                                     epilogue, symmetric, fast, nn_square, want_nn, polite, ldc_pad, Cbuf.ctypes.data,
                                     None if nnbuf is None else nnbuf.ctypes.data)
    assert rc == 0, lib.sharp_last_error()
    return Cbuf, nnbuf


def _gemm_batch(lib, ops, **kw):
    """ops: [(At, Bt)] with Bt None for a symmetric batch -> ([C_t, M x ldc], [nn_t, (ldc / 128) x ldc] or None)"""
    sym = kw.get("symmetric", 0)
    M = [a.shape[1] for a, _ in ops]
    N = [a.shape[1] if sym else b.shape[1] for a, b in ops]
    K = [a.shape[0] for a, _ in ops]
    At = np.concatenate([np.asarray(a, np.float64).ravel() for a, _ in ops])
    Bt = None if sym else np.concatenate([np.asarray(b, np.float64).ravel() for _, b in ops])
    Cbuf, nnbuf = _gemm_batch_raw(lib, M, N, K, At, Bt, **kw)
    Cs, nns, oc, on = [], [], 0, 0
    for m, n in zip(M, N):
        ldc = R.rup(n, 128) if kw.get("ldc_pad", 0) else n
        Cs.append(Cbuf[oc:oc + m * ldc].reshape(m, ldc))
        oc += m * ldc
        if nnbuf is not None:
            nns.append(nnbuf[on:on + ldc // 128 * ldc].reshape(ldc // 128, ldc))
            on += ldc // 128 * ldc
    assert oc == Cbuf.size and (nnbuf is None or on == nnbuf.size)
    return Cs, (nns if nnbuf is not None else None)


def _check_c(Cm, ref, N, what, symmetric=False):
    """the M x N block equals the reference element for element (a NaN equals nothing); the padding columns were not written"""
    ref = np.asarray(ref).astype(np.float64)
    assert _written(Cm[:, :N]).all(), (what, "unwritten elements", np.argwhere(~_written(Cm[:, :N]))[:5])
    bad = np.argwhere(Cm[:, :N] != ref)
    assert bad.size == 0, (what, "first wrong elements (row, col)", bad[:5].tolist(), len(bad))
    assert not _written(Cm[:, N:]).any(), (what, "written beyond column N", np.argwhere(_written(Cm[:, N:]))[:5])
    if symmetric:
        assert np.array_equal(Cm[:, :N], Cm[:, :N].T), what


def _check_nn(nn, ref_nn, n, what):
    slots = (n + 127) // 128
    assert nn.shape[0] == slots and ref_nn.shape == (slots, n)
    assert _written(nn[:, :n]).all(), (what, "slots never written (slot, row)", np.argwhere(~_written(nn[:, :n]))[:5].tolist())
    bad = np.argwhere(nn[:, :n] != ref_nn)
    assert bad.size == 0, (what, "first wrong minima (slot, row)", bad[:5].tolist(), len(bad))
    assert not _written(nn[:, n:]).any(), (what, "rows >= n written")


@functools.lru_cache(maxsize=None)
def _int_case(M, N, K):
    A, B = R.int_operand(1, K, M), R.int_operand(2, K, N)
    return A, B, R.gemm_ref(A, B)


@functools.lru_cache(maxsize=None)
def _int_sym_case(n, K):
    A = R.int_operand(3, K, n)
    return A, R.gemm_ref(A, A)


def _sym_k(n):
    return {1: 1, 2: 3, 5: 4}.get(n, 47)


@pytest.mark.parametrize("ldc_pad", [0, 1])
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("M,N,K", R.GEMM_SHAPES)
def test_integer_product_is_exact(lib, fast, ldc_pad, M, N, K):
    """integers in [-8, 8]: every partial sum is an integer below 2^53 in any order, so a dropped, repeated or misplaced k tile or
    output tile cannot hide behind a tolerance"""
    A, B, ref = _int_case(M, N, K)
    (Cm,), _ = _gemm_batch(lib, [(A, B)], fast=fast, ldc_pad=ldc_pad)
    assert Cm.shape == (M, R.rup(N, 128) if ldc_pad else N)
    _check_c(Cm, ref, N, (M, N, K, fast, ldc_pad))


@pytest.mark.parametrize("ldc_pad", [0, 1])
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("n", R.SYM_SIZES)
def test_symmetric_integer_product_is_exact_and_mirrored(lib, fast, ldc_pad, n):
    A, ref = _int_sym_case(n, _sym_k(n))
    (Cm,), _ = _gemm_batch(lib, [(A, None)], symmetric=1, fast=fast, ldc_pad=ldc_pad)
    _check_c(Cm, ref, n, (n, fast, ldc_pad), symmetric=True)


@functools.lru_cache(maxsize=None)
def _epi_case(M, N, K):
    At, Bt, same = R.eighths_operands(3, K, M, N)
    return At, Bt, same, {e: R.gemm_ref(At, Bt, e).astype(np.float64) for e in (1, 2)}


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("M,N,K", R.EPI_CASES)
def test_epilogues_are_exact_on_eighths(lib, fast, M, N, K):
    """operands in eighths: v is a multiple of 1/64, so the clamps (reached at +1 and at -1: test_linalg_cpu.py), 1 - v and the
    diagonal are exact"""
    At, Bt, same, refs = _epi_case(M, N, K)
    for e in (1, 2):
        for sym in ([0, 1] if same else [0]):
            (Cm,), _ = _gemm_batch(lib, [(At, None if sym else Bt)], epilogue=e, symmetric=sym, fast=fast, ldc_pad=1)
            _check_c(Cm, refs[e], N, (M, N, K, fast, e, sym), symmetric=bool(sym))
            assert np.all(np.diag(Cm[:, :N]) == (0.0 if e == 1 else 1.0))


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("K", [17, 391])
@pytest.mark.parametrize("M,N", [s[:2] for s in R.GEMM_SHAPES])
def test_continuous_product_within_the_dot_product_bound(lib, fast, K, M, N):
    rng = np.random.default_rng([M, N, K])
    At, Bt = rng.standard_normal((K, M)), rng.standard_normal((K, N))
    (Cm,), _ = _gemm_batch(lib, [(At, Bt)], fast=fast, ldc_pad=1)
    assert _written(Cm[:, :N]).all() and not _written(Cm[:, N:]).any()
    err, bound = np.abs(Cm[:, :N] - R.gemm_ref(At, Bt)), R.gemm_bound(At, Bt)
    print((M, N, K, fast), "max error / bound", float((err / bound).max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("n", R.NN_SIZES)
def test_row_minima_equal_the_reference(lib, n):
    """GemmTask::nn of the distance GEMM as the agglomeration runs it (fast, symmetric, epilogue 1), plain and squared: (a) on operands
    in eighths C and nn equal the reference's bit for bit; (b) on continuous unit columns nn equals nn_ref of the C THE SAME CALL
    returned -- one call's two outputs, not two paths.  Every slot of every row is written, the rows of the padding are not, and a slot
    whose only column is the row itself holds 1e300."""
    A, U = R.nn_exact_operand(7, n), R.unit_columns(8, R.NN_K, n)
    ref = R.gemm_ref(A, A, 1).astype(np.float64)
    ref_u, bound_u = R.gemm_ref(U, U, 1), R.gemm_bound(U, U) + 2 * R.EPS53          # (+ the rounding of 1 - v, |1 - v| <= 2)
    for square in (0, 1):
        kw = dict(epilogue=1, symmetric=1, fast=1, nn_square=square, want_nn=1, ldc_pad=1)
        (Cm,), (nn,) = _gemm_batch(lib, [(A, None)], **kw)
        _check_c(Cm, ref, n, ("exact", n), symmetric=True)
        _check_nn(nn, R.nn_ref(ref, n, square), n, ("exact", n, square))
        (Cu,), (nnu,) = _gemm_batch(lib, [(U, None)], **kw)
        assert _written(Cu[:, :n]).all() and not _written(Cu[:, n:]).any() and np.array_equal(Cu[:, :n], Cu[:, :n].T)
        assert np.all(np.abs(Cu[:, :n] - ref_u) <= bound_u)
        _check_nn(nnu, R.nn_ref(Cu, n, square), n, ("continuous", n, square))
        if n == 129:
            assert nn[1, 128] == R.NN_INF and nnu[1, 128] == R.NN_INF
        assert nnu[:, :n].min() > 0.0 and nn[:, :n].min() > 0.0        # the zero diagonal never enters


def _sym_batch(count, largest_first, seed):
    """count symmetric tasks: 520 first or last, the others drawn from the ragged sizes, each with its own K"""
    rng = np.random.default_rng([count, int(largest_first), seed])
    sizes = [int(v) for v in rng.choice([5, 129, 200, 385], size=count - 1)]
    sizes = [520] + sizes if largest_first else sizes + [520]
    return [(n, int(k)) for n, k in zip(sizes, rng.choice([4, 30, 47], size=count))]


@pytest.mark.parametrize("largest_first", [True, False])
@pytest.mark.parametrize("count", [1, 7, 8, 9, 17])
def test_batch_of_symmetric_tasks_on_the_fast_kernel(lib, count, largest_first):
    """the block -> (task, tile) map of gemm_tn_f64_fast_kernel: groups of eight tasks, tiles_max from the largest task while the
    smaller ones return early, count % 8 != 0, the upper-triangle walk; C and nn of every task, exactly"""
    shapes = _sym_batch(count, largest_first, 5)
    cases = [_int_sym_case(n, K) for n, K in shapes]
    Cs, nns = _gemm_batch(lib, [(A, None) for A, _ in cases], symmetric=1, fast=1, want_nn=1, ldc_pad=1)
    for t, ((n, K), (A, ref)) in enumerate(zip(shapes, cases)):
        _check_c(Cs[t], ref, n, ("task", t, n, K), symmetric=True)
        _check_nn(nns[t], R.nn_ref(ref, n, 0), n, ("task", t, n, K))


_RECT = [(100, 90, 17), (300, 600, 4), (129, 128, 33), (1, 257, 16), (257, 1, 5), (128, 129, 47), (64, 385, 30), (200, 200, 1), (385, 64, 31)]


@pytest.mark.parametrize("ldc_pad", [0, 1])
@pytest.mark.parametrize("fast", [0, 1])
def test_batch_of_unequal_rectangular_tasks(lib, fast, ldc_pad):
    """nine tasks with unequal (M, N, K), one tile beside 3 x 5 tiles: the fast kernel's L / ntn, L % ntn and the generic kernel's
    blockIdx.z batches under a grid sized by the largest M and the largest N, which belong to different tasks"""
    assert max(m for m, _, _ in _RECT) == 385 and max(n for _, n, _ in _RECT) == 600
    cases = [_int_case(*s) for s in _RECT]
    Cs, _ = _gemm_batch(lib, [(A, B) for A, B, _ in cases], fast=fast, ldc_pad=ldc_pad)
    for t, (s, (_, _, ref)) in enumerate(zip(_RECT, cases)):
        _check_c(Cs[t], ref, s[1], ("task", t, s, fast, ldc_pad))


def test_batch_of_symmetric_tasks_on_the_generic_kernel(lib):
    shapes = [(5, 4), (129, 30), (64, 16), (200, 47), (1, 1), (65, 17), (385, 4), (128, 33), (2, 3)]
    cases = [_int_sym_case(n, K) for n, K in shapes]
    Cs, _ = _gemm_batch(lib, [(A, None) for A, _ in cases], symmetric=1, fast=0, ldc_pad=1)
    for t, ((n, K), (_, ref)) in enumerate(zip(shapes, cases)):
        _check_c(Cs[t], ref, n, ("task", t, n, K), symmetric=True)


def test_generic_batch_beyond_one_launch(lib):
    """65 537 tasks of 1 x 1 x 1: gemm_tn_f64_batched's second launch (blockIdx.z holds 65 535)"""
    count = 65537
    rng = np.random.default_rng(65537)
    a, b = rng.integers(-8, 9, size=count), rng.integers(-8, 9, size=count)
    ones = np.ones(count, np.int32)
    for ldc_pad in (0, 1):
        Cbuf, _ = _gemm_batch_raw(lib, ones, ones, ones, a.astype(np.float64), b.astype(np.float64), ldc_pad=ldc_pad)
        Cm = Cbuf.reshape(count, -1)
        assert Cm.shape[1] == (128 if ldc_pad else 1)
        bad = np.flatnonzero(Cm[:, 0] != (a * b).astype(np.float64))
        assert bad.size == 0, ("first wrong tasks", bad[:5].tolist(), len(bad))
        assert not _written(Cm[:, 1:]).any()


def test_sliced_launches_give_the_unsliced_bits(lib):
    """a "polite" batch (Ctx::polite) goes out in slices of SHARP_GEMM_SLICE workgroups per CU: with 1 per CU, 24 tasks x 15 tiles = 360
    workgroups need more than one launch with block0 != 0.  C and nn equal the reference and, bit for bit, the unsliced call's."""
    import torch

    sizes = [520, 5, 129, 200, 385, 520, 385, 200] * 3
    assert len(sizes) * 15 > torch.cuda.get_device_properties(0).multi_processor_count       # more workgroups than one slice holds
    cases = [_int_sym_case(n, 30) for n in sizes]
    ops = [(A, None) for A, _ in cases]
    kw = dict(symmetric=1, fast=1, want_nn=1, ldc_pad=1)
    plain_c, plain_nn = _gemm_batch(lib, ops, polite=0, **kw)
    old = os.environ.get("SHARP_GEMM_SLICE")
    os.environ["SHARP_GEMM_SLICE"] = "1"
    try:
        assert lib.sharp_reload_options() == 0
        sliced_c, sliced_nn = _gemm_batch(lib, ops, polite=1, **kw)
    finally:
        if old is None:
            del os.environ["SHARP_GEMM_SLICE"]
        else:
            os.environ["SHARP_GEMM_SLICE"] = old
        assert lib.sharp_reload_options() == 0
    for t, (n, (_, ref)) in enumerate(zip(sizes, cases)):
        _check_c(sliced_c[t], ref, n, ("sliced task", t, n), symmetric=True)
        _check_nn(sliced_nn[t], R.nn_ref(ref, n, 0), n, ("sliced task", t, n))
        _check_c(plain_c[t], ref, n, ("task", t, n), symmetric=True)
        assert np.array_equal(sliced_c[t].view(np.uint64), plain_c[t].view(np.uint64))
        assert np.array_equal(sliced_nn[t].view(np.uint64), plain_nn[t].view(np.uint64))


def test_batch_entry_refuses_bad_combinations_by_name(lib):
    one = np.ones(1, np.int32)
    x = np.ones(1)
    out = np.zeros(128)

    def call(**kw):
        a = dict(count=1, M=one, N=one, K=one, Bt=x, epilogue=0, symmetric=0, fast=0, nn_square=0, want_nn=0, polite=0, ldc_pad=0, nn=None)
        a.update(kw)
        p = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        rc = lib.sharp_gemm_tn_f64_batch(a["count"], p(a["M"]), p(a["N"]), p(a["K"]), x.ctypes.data, p(a["Bt"]), a["epilogue"], a["symmetric"],
                                         a["fast"], a["nn_square"], a["want_nn"], a["polite"], a["ldc_pad"], out.ctypes.data, p(a["nn"]))
        return rc, lib.sharp_last_error().decode()

    assert call()[0] == 0
    for kw, word in [(dict(count=0), "count"), (dict(Bt=None), "null Bt"), (dict(epilogue=3), "epilogue"),
                     (dict(want_nn=1, nn=out, fast=1, symmetric=1), "want_nn needs"), (dict(want_nn=1, fast=1, symmetric=1, ldc_pad=1), "null nn"),
                     (dict(nn_square=1), "nn_square"), (dict(polite=1), "polite"), (dict(symmetric=1, N=2 * one), "M == N"),
                     (dict(K=0 * one), "at least 1")]:
        rc, msg = call(**kw)
        assert rc != 0 and "sharp_gemm_tn_f64_batch" in msg and word in msg, (kw, rc, msg)


# ---- row preparation --------------------------------------------------------------------------------------------------------------------
def _row_prep_batch(lib, tasks, all_feature_rows):
    """tasks: [(src (n x lds), p, mode)] -> per task {Cr (n x p), Ct (p_pad x nld), nrm (n), D (nld x nld)}, every buffer whole"""
    n = np.array([s.shape[0] for s, _, _ in tasks], np.int32)
    lds = np.array([s.shape[1] for s, _, _ in tasks], np.int64)
    p = np.array([q for _, q, _ in tasks], np.int32)
    mode = np.array([m for _, _, m in tasks], np.int32)
    src = np.concatenate([np.ascontiguousarray(s, np.float64).ravel() for s, _, _ in tasks])
    nld, p_pad = R.rup(n.astype(np.int64), 128), R.rup(p.astype(np.int64), 16)
    Cr, Ct, nrm, D = np.zeros(int((n * p.astype(np.int64)).sum())), np.zeros(int((p_pad * nld).sum())), np.zeros(int(n.sum())), np.zeros(int((nld * nld).sum()))
    rc = lib.sharp_row_prep_batch(len(tasks), n.ctypes.data, p.ctypes.data, lds.ctypes.data, mode.ctypes.data, src.ctypes.data, int(all_feature_rows),
                                  Cr.ctypes.data, Ct.ctypes.data, nrm.ctypes.data, D.ctypes.data)
    assert rc == 0, lib.sharp_last_error()
    out, o = [], [0, 0, 0, 0]
    for t in range(len(tasks)):
        sz = [int(n[t]) * int(p[t]), int(p_pad[t] * nld[t]), int(n[t]), int(nld[t] * nld[t])]
        out.append({"Cr": Cr[o[0]:o[0] + sz[0]].reshape(int(n[t]), int(p[t])), "Ct": Ct[o[1]:o[1] + sz[1]].reshape(int(p_pad[t]), int(nld[t])),
                    "nrm": nrm[o[2]:o[2] + sz[2]], "D": D[o[3]:o[3] + sz[3]].reshape(int(nld[t]), int(nld[t]))})
        o = [a + b for a, b in zip(o, sz)]
    assert o == [Cr.size, Ct.size, nrm.size, D.size]
    return out


@functools.lru_cache(maxsize=None)
def _prep_ref(kind, n, p, mode):
    """(source without padding columns, reference, (tol Cr, tol nrm)) -- computed once, shared, never changed"""
    src = {"rows": lambda: R.feature_rows(11, n, p, p)[:, :p], "sim": lambda: R.similarity(12, n), "dist": lambda: R.distances(13, n)}[kind]()
    ref = R.row_prep_ref(src, n, p, mode)
    return src, ref, (R.row_prep_bounds(ref, p, mode) if mode != 2 else None)


def _check_prep(got, kind, n, p, mode, what):
    src, ref, tols = _prep_ref(kind, n, p, mode)
    Cr, Ct, nrm, D = got["Cr"], got["Ct"], got["nrm"], got["D"]
    if mode == 2:
        assert not _written(Cr).any() and not _written(Ct).any() and not _written(nrm).any(), (what, "mode 2 touched Cr / Ct / nrm")
    else:
        assert _written(Cr).all() and _written(nrm).all() and _written(Ct).all(), (what, "unwritten elements of Cr / nrm / Ct")
        tol, tol_n = tols
        err = np.abs(Cr - ref["Cr"])
        print(what, "Cr: max error", float(err.max()), "smallest bound", float(tol.min()), "| nrm: max error", float(np.abs(nrm - ref["nrm"]).max()))
        assert np.all(err <= tol), (what, "Cr", np.argwhere(err > tol)[:5].tolist())
        assert np.all(np.abs(nrm - ref["nrm"]) <= tol_n), (what, "nrm")
        assert np.array_equal(Ct[:p, :n].view(np.uint64), np.ascontiguousarray(Cr.T).view(np.uint64)), (what, "Ct[:p, :n] is not Cr^T")
        assert np.all(np.abs(Ct[:p, :n] - ref["Cr"].T) <= tol.T), (what, "Ct")
        assert np.all(Ct[p:, :] == 0.0) and np.all(Ct[:, n:] == 0.0), (what, "the padding of Ct is not zero",
                                                                        np.argwhere(~(Ct[p:, :] == 0.0))[:3].tolist(), np.argwhere(~(Ct[:, n:] == 0.0))[:3].tolist())
    if mode == 0:
        assert not _written(D).any(), (what, "mode 0 touched D")
    else:
        assert _written(D[:n, :n]).all(), (what, "unwritten elements of D")
        bad = np.argwhere(D[:n, :n] != ref["D"])
        assert bad.size == 0, (what, "D: first wrong elements", bad[:5].tolist(), len(bad))
        assert np.all(np.diag(D[:n, :n]) == 0.0)
        assert not _written(D[n:, :]).any() and not _written(D[:, n:]).any(), (what, "D written beyond n x n")


def _rows_src(n, p, pad=0):
    X = R.feature_rows(11, n, p, p + pad)
    assert np.array_equal(X[:, :p], _prep_ref("rows", n, p, 0)[0])
    return X


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n,p", R.ROW_SHAPES)
def test_feature_rows_single_task(lib, n, p, pad):
    """mode 0 through each launch form: p <= 512 with all_feature_rows (row_prep_t_kernel alone) and without (the other two kernels are
    launched and have to leave the task alone), p > 512 on the general path; lds == p and lds > p"""
    X = _rows_src(n, p, pad)
    outs = []
    for afr in ([1, 0] if p <= 512 else [0]):
        (got,) = _row_prep_batch(lib, [(X, p, 0)], afr)
        _check_prep(got, "rows", n, p, 0, ("rows", n, p, pad, afr))
        assert np.all(got["nrm"] == 1.0)
        outs.append(got)
    if len(outs) == 2:
        assert all(np.array_equal(outs[0][k].view(np.uint64), outs[1][k].view(np.uint64)) for k in ("Cr", "Ct", "nrm", "D"))


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", R.SIM_SIZES)
def test_similarity_single_task(lib, n, pad):
    """mode 1: D = 1 - S from the LOWER triangle (the upper one is perturbed), centred rows, their norms"""
    S = np.full((n, n + pad), 1.0e6)
    S[:, :n] = _prep_ref("sim", n, n, 1)[0]
    (got,) = _row_prep_batch(lib, [(S, n, 1)], 0)
    _check_prep(got, "sim", n, n, 1, ("similarity", n, pad))


@pytest.mark.parametrize("n", R.DIST_SIZES)
def test_distance_single_task(lib, n):
    """mode 2: the rows as they are with a zero diagonal; nothing else is touched"""
    (got,) = _row_prep_batch(lib, [(_prep_ref("dist", n, n, 2)[0], n, 2)], 0)
    _check_prep(got, "dist", n, n, 2, ("distance", n))


def test_mixed_batch_where_skip_fused_deals_the_tasks(lib):
    """max_p <= 512 and not every task has feature rows: row_prep_t_kernel takes the two mode-0 tasks, row_prep_kernel and
    transpose_kernel the other two and must skip the first pair"""
    tasks = [("rows", 200, 30, 0), ("sim", 150, 150, 1), ("dist", 97, 97, 2), ("rows", 17, 512, 0)]
    got = _row_prep_batch(lib, [(_prep_ref(*t)[0], t[2], t[3]) for t in tasks], 0)
    for g, t in zip(got, tasks):
        _check_prep(g, *t, ("mixed", t))


def test_short_rows_beside_long_rows_take_the_register_path(lib):
    """max_p > 512: nothing is fused, and the (200, 30) task goes through row_prep_kernel's register path and transpose_kernel.  Its Cr
    is checked against the reference and -- linalg.hip states that the three mode-0 paths do the same operations in the same order --
    must ALSO have the bits row_prep_t_kernel gives it in a batch of its own"""
    tasks = [("rows", 200, 30, 0), ("rows", 40, 513, 0)]
    got = _row_prep_batch(lib, [(_prep_ref(*t)[0], t[2], t[3]) for t in tasks], 0)
    for g, t in zip(got, tasks):
        _check_prep(g, *t, ("unfused", t))
    (alone,) = _row_prep_batch(lib, [(_prep_ref(*tasks[0])[0], 30, 0)], 1)
    _check_prep(alone, *tasks[0], ("fused", tasks[0]))
    assert np.array_equal(alone["Cr"].view(np.uint64), got[0]["Cr"].view(np.uint64))
    assert np.array_equal(alone["Ct"].view(np.uint64), got[0]["Ct"].view(np.uint64))


def test_row_prep_entry_refuses_bad_combinations_by_name(lib):
    x = np.ones(16)
    out = np.zeros(128 * 128)

    def call(n, p, lds, mode, afr, count=1):
        a = [np.array([v], t) for v, t in ((n, np.int32), (p, np.int32), (lds, np.int64), (mode, np.int32))]
        rc = lib.sharp_row_prep_batch(count, *[v.ctypes.data for v in a], x.ctypes.data, afr, *([out.ctypes.data] * 4))
        return rc, lib.sharp_last_error().decode()

    assert call(2, 3, 3, 0, 1)[0] == 0
    for args, word in [((2, 3, 3, 0, 0, 0), "count"), ((2, 3, 2, 0, 0), "lds >= p"), ((2, 3, 3, 3, 0), "mode"), ((2, 3, 3, 1, 0), "n == p"),
                       ((3, 3, 3, 1, 1), "all_feature_rows")]:
        rc, msg = call(*args)
        assert rc != 0 and "sharp_row_prep_batch" in msg and word in msg, (args, rc, msg)
