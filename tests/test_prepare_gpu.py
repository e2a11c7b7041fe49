"""The input preparation stage (csrc/prepare.hip through sharp_tsne_prepare / tsne._prepare) on its own: centring, scaling, PCA,
normalisation, at the row counts where its slab counts change, the column counts where its tiles are ragged, and its refusals.
tests/_prepare_ref.py holds the reference, the exact designs and the bounds (derived there, not fitted).

Every test prints "prepare-bound <case>: <largest error / bound>" before it asserts; profiles/prepare_tests_bounds.txt is those lines
of one run.  Bit-for-bit cases print 0 or fail."""
import ctypes as C
import functools

import numpy as np
import pytest

import _prepare_ref as ref

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def T():
    import sharp_amd
    from sharp_amd import tsne

    sharp_amd.init(0)
    return tsne


def _report(case, ratio):
    print(f"prepare-bound {case}: {ratio:.3g}")


def _same(case, got, want):
    """bit for bit (a zero of either sign is a zero)"""
    assert got.shape == want.shape, (case, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    _report(case, 0.0 if bad.size == 0 else np.inf)
    assert bad.size == 0, f"{case}: {bad.size} entries differ, first at {np.unravel_index(bad[0], got.shape)}: " \
                          f"{got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


def _prepare_ld(X, ld, pad, **kw):
    """sharp_tsne_prepare by ctypes on rows ld apart, the padding filled with `pad`"""
    from sharp_amd._lib import check, f64, lib

    n, d = X.shape
    buf = np.full((n, ld), pad, np.float64)
    buf[:, :d] = X
    out = np.zeros((n, d))
    dd = C.c_int()
    check(lib().sharp_tsne_prepare(f64(buf), n, d, ld, int(kw.get("pca", 1)), int(kw.get("initial_dims", 50)), int(kw.get("pca_center", 1)),
                                   int(kw.get("pca_scale", 0)), int(kw.get("normalize", 1)), f64(out), C.byref(dd)))
    return np.ascontiguousarray(out.reshape(-1)[: n * dd.value].reshape(n, dd.value))


# ---- bit for bit on the exact design -------------------------------------------------------------------------------------------------
# n: the column_stat slab-count edges (min(256, n / 256) slabs of ceil(n / slabs) rows); d: one thread per column, 256 per block
NORMALIZE_CASES = [(2, 1), (2, 600), (255, 17), (256, 257), (511, 3), (512, 600), (513, 17), (513, 257), (65535, 1), (65536, 3), (65537, 3)]


@pytest.mark.parametrize("n,d", NORMALIZE_CASES)
def test_normalize_alone_is_exact_on_the_design(T, n, d):
    X, o = ref.design(n, d, offsets=True)
    Xc, _ = ref.check_design(X, o, center=True)
    assert np.abs(Xc).max() > 0
    want = Xc / np.abs(Xc).max()
    _same(f"normalize n={n} d={d}", T._prepare(X, pca=False, normalize=True), want)
    _same(f"identity n={n} d={d}", T._prepare(X, pca=False, normalize=False), X)


# n: the Gram slab-count edges (min(64, n / 512) slabs, the last one ragged) and column_stat's; d: ragged symmetric tiles.  A covering
# set, not the product: every n, every d and every kind of initial_dims at least once, with d <= n // 2 so that the design uses
# every column, and n d <= 3 * 65 537.  (No n leaves a last slab of one row: ceil(n / slabs) >= 256 > slabs.)
PCA_CASES = [(3, 1, "d+5"), (3, 1, "1"), (511, 2, "d-1"), (511, 64, "d"), (512, 3, "d"), (512, 17, "1"), (1023, 5, "d+5"),
             (1023, 257, "d-1"), (1024, 16, "d"), (1024, 257, "d+5"), (1025, 17, "d-1"), (1025, 33, "d"), (1537, 33, "d+5"),
             (1537, 64, "1"), (1537, 257, "d"), (32767, 3, "d"), (32768, 5, "d-1"), (33001, 2, "d+5"), (33001, 5, "1")]


def _idims(d, kind):
    return {"1": 1, "d-1": d - 1, "d": d, "d+5": d + 5}[kind]


@pytest.mark.parametrize("center", [1, 0])
@pytest.mark.parametrize("n,d,kind", PCA_CASES)
def test_pca_is_exact_on_the_design(T, n, d, kind, center):
    """the Gram matrix is exactly diagonal with distinct entries: the components are the centred columns themselves, in descending
    order of their sum of squares, unchanged (the unit vector's one component is the largest and positive: no column is negated)"""
    idims = _idims(d, kind)
    X, o = ref.design(n, d, offsets=bool(center))
    Xc, dg = ref.check_design(X, o, center=bool(center))
    want = ref.design_expected(Xc, dg, idims)
    assert want.shape[1] == min(idims, d)
    case = f"pca n={n} d={d} initial_dims={idims} center={center}"
    got = T._prepare(X, pca=True, initial_dims=idims, pca_center=bool(center), normalize=False)
    _same(case, got, want)
    # normalised: the column means are exactly zero (+- pairs), one division by the largest |entry|
    _same(case + " normalize", T._prepare(X, pca=True, initial_dims=idims, pca_center=bool(center), normalize=True), want / np.abs(want).max())


@pytest.mark.parametrize("center", [1, 0])
@pytest.mark.parametrize("n,d,k", [(513, 5, 3), (1537, 33, 10), (65537, 3, 2), (514, 257, 4)])
def test_scale_equals_prescaled_input(T, n, d, k, center):
    """pca_scale = 1 on integers whose mean and sum of squares are exact equals no scaling of Z = (X - mu) / sd made in numpy:
    sd = sqrt(SS / (n - 1)) about the centre used -- the mean, or zero without centring -- is then the same double on both sides
    (one division, one root, both correctly rounded), and so is every x / sd."""
    X, o = ref.design(n, d, offsets=True)
    X = X + ref.dense_pairs(n, d, seed=n + d)
    assert np.array_equal(X.astype(LD).sum(0), LD(n) * o.astype(LD))
    mu = o if center else np.zeros(d)
    dev = X - mu
    ss = (dev * dev).sum(0)
    assert np.array_equal(ss.astype(LD), (dev.astype(LD) ** 2).sum(0)) and ss.max() < 2.0 ** 53 and ss.min() > 0
    sd = np.sqrt(ss / float(n - 1))
    Z = dev / sd
    for norm in (False, True):
        a = T._prepare(X, pca=True, initial_dims=k, pca_center=bool(center), pca_scale=True, normalize=norm)
        b = T._prepare(Z, pca=True, initial_dims=k, pca_center=False, pca_scale=False, normalize=norm)
        _same(f"scale n={n} d={d} center={center} normalize={int(norm)}", a, b)
    # and the scaled columns have the unit sd the convention promises: with k = d the scores' total sum of squares is (n - 1) d, within
    # the entries' gamma_{n+8} (squared: twice), the projection's gamma_d and the solver's ||V^T V - I||_2 <= d * (c d u) (test_eigen_cpu)
    full = T._prepare(X, pca=True, initial_dims=d, pca_center=bool(center), pca_scale=True, normalize=False)
    tot = float((full.astype(LD) ** 2).sum())
    tol = (2 * ref.gamma(n + 8) + 2 * ref.gamma(d) + 2 * ref.C_EIGEN * d * d * ref.U) * ref.SAFETY * (n - 1) * d
    _report(f"scale total n={n} d={d} center={center}", abs(tot - (n - 1) * d) / tol)
    assert abs(tot - (n - 1) * d) <= tol


@pytest.mark.parametrize("kw", [dict(pca=0, normalize=1), dict(pca=1, initial_dims=4, normalize=0), dict(pca=1, initial_dims=20, pca_scale=1, normalize=1)])
def test_padding_is_never_read_and_calls_repeat(T, kw):
    X = ref.spectrum_data(700, 9, 6, seed=31)
    a = _prepare_ld(X, 9, 0.0, **kw)
    _same(f"ld = d + 3 with NaN padding {kw}", _prepare_ld(X, 12, np.nan, **kw), a)
    _same(f"second call {kw}", _prepare_ld(X, 9, 0.0, **kw), a)
    _same(f"_prepare {kw}", T._prepare(X, pca=bool(kw["pca"]), initial_dims=kw.get("initial_dims", 50), pca_scale=bool(kw.get("pca_scale", 0)),
                                       normalize=bool(kw["normalize"])), a)


# ---- continuous data against the reference -------------------------------------------------------------------------------------------
SHAPES = [(40, 100, 10), (700, 33, 33), (5000, 120, 30), (3000, 600, 50), (2049, 7, 2)]
KINDS = [("gauss", 1, 0), ("gauss", 1, 1), ("gauss", 0, 0), ("gauss", 0, 1), ("shift1e6", 1, 0), ("shift1e6", 1, 1), ("scales1e6", 1, 1),
         ("scales1e6", 0, 1)]


@functools.lru_cache(maxsize=2)
def _data(n, d, k, kind):
    X = ref.spectrum_data(n, d, k + 2, seed=1000 + n + d)
    if kind == "shift1e6":
        X = X + 1e6
    if kind == "scales1e6":
        X = X * 10.0 ** np.random.default_rng(n).permutation(np.linspace(-3, 3, d))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=2)
def _reference(n, d, k, kind, center, scale):
    X = _data(n, d, k, kind)
    R = ref.pca(X, k, bool(center), bool(scale))
    b, parts = ref.pca_bound(X, R, center, scale)
    return X, R, b, parts


@pytest.mark.parametrize("kind,center,scale", KINDS)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_pca_scores_within_the_derived_bound(T, n, d, k, kind, center, scale):
    X, R, b, parts = _reference(n, d, k, kind, center, scale)
    case = f"scores n={n} d={d} k={k} {kind} center={center} scale={scale}"
    gaps = ref.relative_gaps(R["w"], k)
    assert gaps.min() >= 1e-3, (case, gaps.min())
    S = R["scores"]
    got = T._prepare(X, pca=True, initial_dims=k, pca_center=bool(center), pca_scale=bool(scale), normalize=False)
    assert got.shape == (n, k)
    err = np.abs(got.astype(LD) - S).astype(np.float64)
    ratio = float((err / b).max())
    _report(case, ratio)
    print(f"    largest error {err.max():.3g} of scores up to {float(np.abs(S).max()):.3g}; ||E|| / ||G|| = {parts['E'] / parts['g2']:.3g} "
          f"(Gram {parts['e_gram'] / parts['g2']:.3g}, solvers {parts['e_solver'] / parts['g2']:.3g}), largest vector bound {parts['dv'].max():.3g}")
    assert parts["dv"].max() < 1e-3, "the bound says something"
    assert ratio <= 1.0
    gotn = T._prepare(X, pca=True, initial_dims=k, pca_center=bool(center), pca_scale=bool(scale), normalize=True)
    bn = ref.normalize_bound(S, b)
    rn = float((np.abs(gotn.astype(LD) - ref.normalize(S)).astype(np.float64) / bn).max())
    _report(case + " normalize", rn)
    assert np.abs(gotn).max() == 1.0
    assert rn <= 1.0
    if n >= d:
        # the rotation itself: V = lstsq(Xc, out).  A consistent system: numpy's solution errs by about u cond(Xc) (Golub & Van Loan
        # §5.3.7, zero residual), taken as d gamma_n cond; the scores' error adds ||b_j||_2 / sigma_min.
        Xc = R["Xc"].astype(np.float64)
        sv = np.linalg.svd(Xc, compute_uv=False)
        assert sv[-1] > 1e-6 * sv[0]
        V = np.linalg.lstsq(Xc, got, rcond=None)[0]
        tv = np.sqrt((b * b).sum(0)).max() / sv[-1] + d * ref.gamma(n) * sv[0] / sv[-1]
        orth = np.abs(V.T @ V - np.eye(k)).max()
        _report(case + " V^T V = I", orth / (2 * tv + tv * tv + ref.gamma(d)))
        assert orth <= 2 * tv + tv * tv + ref.gamma(d)
        a = np.sort(np.abs(V), axis=0)
        decided = a[-1] - a[-2] > 2 * tv if d > 1 else np.ones(k, bool)
        print(f"    sign rule decided on {int(decided.sum())} of {k} vectors (recovered V within {tv:.3g})")
        assert decided.any()
        top = V[np.abs(V).argmax(0), np.arange(k)]
        assert np.all(top[decided] > 0), "sign rule: the largest |component| of every vector is positive"
        assert np.abs(V - R["V"]).max() <= parts["dv"].max() + tv


# ---- degenerate spectra --------------------------------------------------------------------------------------------------------------
def test_two_equal_leading_eigenvalues(T):
    n, d, k = 600, 12, 6
    X = ref.spectrum_data(n, d, k + 2, seed=77, equal_pair=True)
    R = ref.pca(X, k, True, False)
    w = R["w"]
    assert (w[0] - w[1]) / w[0] < 1e-12 and ref.relative_gaps(w[1:], k - 1).min() >= 1e-3
    b, parts = ref.pca_bound(X, R, 1, 0)
    got = T._prepare(X, pca=True, initial_dims=k, normalize=False)
    # the pair: any basis of its plane.  Yu, Wang & Samworth, Theorem 2: ||sin Theta||_F <= 2 sqrt(2) ||E||_2 / gap for a plane, and
    # ||P^ - P||_F = sqrt(2) ||sin Theta||_F; entry (r, s) of Xc (P^ - P) Xc^T is within ||xc_r|| ||xc_s|| of that
    Xc = R["Xc"].astype(np.float64)
    rown = np.sqrt((Xc * Xc).sum(1))
    dP = 4 * parts["E"] / (w[1] - w[2])
    S = R["scores"][:, :2].astype(np.float64)
    bp = ref.SAFETY * (np.outer(rown, rown) * dP + 4 * ref.gamma(d + n + 8) * np.outer(rown, rown))
    rp = float((np.abs(got[:, :2] @ got[:, :2].T - S @ S.T) / bp).max())
    _report("equal pair: projector", rp)
    assert dP < 1e-6 and rp <= 1.0
    ro = float((np.abs(got[:, 2:].astype(LD) - R["scores"][:, 2:]).astype(np.float64) / b[:, 2:]).max())
    _report("equal pair: other components", ro)
    assert parts["dv"][2:].max() < 1e-3 and ro <= 1.0


def test_components_past_the_rank_are_zero(T):
    n, d, k = 40, 100, 60
    X = ref.spectrum_data(n, d, 60, seed=78)
    R = ref.pca(X, k, True, False)
    rank = n - 1
    assert R["w"][rank - 1] > 1e-3 * R["w"][0] and abs(R["w"][rank]) < 1e-12 * R["w"][0]
    b, parts = ref.pca_bound(X, R, 1, 0)
    got = T._prepare(X, pca=True, initial_dims=k, normalize=False)
    assert got.shape == (n, k)
    r1 = float((np.abs(got[:, :rank].astype(LD) - R["scores"][:, :rank]).astype(np.float64) / b[:, :rank]).max())
    _report("past the rank: components within it", r1)
    assert parts["dv"][:rank].max() < 1e-3 and r1 <= 1.0
    zb = max(ref.zero_bound(R, parts, n, d, j) for j in range(rank, k))
    _report("past the rank: zero components", float(np.abs(got[:, rank:]).max() / zb))
    assert zb < 1e-4 * np.abs(got[:, 0]).max()
    assert np.abs(got[:, rank:]).max() <= zb


# ---- refusals, by message, a good call after each -------------------------------------------------------------------------------------
def _good(T):
    X, o = ref.design(64, 3, offsets=True)
    assert np.array_equal(T._prepare(X, pca=True, initial_dims=2, normalize=False), ref.design_expected(*ref.check_design(X, o, True), 2))


def test_refusals(T):
    import sharp_amd

    X = ref.spectrum_data(300, 6, 4, seed=5)
    Xk = X.copy()
    Xk[:, 3] = 7.25
    with pytest.raises(sharp_amd.SharpError, match=r"Rtsne: cannot rescale a constant/zero column to unit variance \(column 4\)"):
        T._prepare(Xk, pca=True, initial_dims=3, pca_center=True, pca_scale=True)
    _good(T)
    Xz = X.copy()
    Xz[:, 5] = 0.0
    with pytest.raises(sharp_amd.SharpError, match=r"cannot rescale a constant/zero column to unit variance \(column 6\)"):
        T._prepare(Xz, pca=True, initial_dims=3, pca_center=False, pca_scale=True)
    _good(T)
    # a constant column that is not zero has a root mean square about zero: without centring it is scaled, not refused
    assert T._prepare(Xk, pca=True, initial_dims=3, pca_center=False, pca_scale=True, normalize=False).shape == (300, 3)
    for bad in (0, -2):
        with pytest.raises(sharp_amd.SharpError, match="Rtsne: initial_dims must be >= 1"):
            T._prepare(X, pca=True, initial_dims=bad)
        _good(T)
    # all rows equal (integers: the mean is exact and every centred entry is zero)
    with pytest.raises(sharp_amd.SharpError, match="Rtsne: the normalised input is all zero or not finite"):
        T._prepare(np.tile(np.array([3.0, -8.0, 1024.0]), (500, 1)), pca=False, normalize=True)
    _good(T)
    # finite input whose column sum overflows: the mean is Inf
    big = np.full((4, 2), 1.7e308)
    big[:, 1] = [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(sharp_amd.SharpError, match="Rtsne: the normalised input is all zero or not finite"):
        T._prepare(big, pca=False, normalize=True)
    _good(T)
    for v in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[17, 2] = v
        with pytest.raises(sharp_amd.SharpError, match=r"Rtsne: the input holds NA / NaN / Inf \(row 18, column 3\)"):
            T._prepare(Xb, pca=False, normalize=True)
        _good(T)


def test_nan_never_reaches_the_pca(T):
    """pca = 1, normalize = 0 has no check of its own inside the stage: a NaN would make the Gram matrix NaN and the solver refuse it
    ("did not converge", tests/test_eigen_cpu.py).  Today no caller lets it in: sharp_tsne_prepare and sharp_tsne refuse it on the
    host before the upload ("Rtsne: the input holds NA / NaN / Inf (row, column)"), sharp_umap likewise, and snn / louvain in Python."""
    import sharp_amd

    X = ref.spectrum_data(400, 8, 6, seed=6)
    X[123, 4] = np.nan
    with pytest.raises(sharp_amd.SharpError, match=r"Rtsne: the input holds NA / NaN / Inf \(row 124, column 5\)"):
        T._prepare(X, pca=True, initial_dims=5, normalize=False)
    with pytest.raises(sharp_amd.SharpError, match=r"Rtsne: the input holds NA / NaN / Inf \(row 124, column 5\)"):
        sharp_amd.Rtsne(X, initial_dims=5, perplexity=10, max_iter=5, normalize=False)
    with pytest.raises(sharp_amd.SharpError, match=r"umap: the input holds NA / NaN / Inf \(row 124, column 5\)"):
        sharp_amd.umap(X, pca=5, n_epochs=5)
    with pytest.raises(sharp_amd.SharpError, match=r"snn: the input holds NA / NaN / Inf \(row 124, column 5\)"):
        sharp_amd.snn(X, pca=5)
    with pytest.raises(sharp_amd.SharpError, match=r"louvain: the input holds NA / NaN / Inf \(row 124, column 5\)"):
        sharp_amd.louvain(X, pca=5)
    _good(T)


# ---- the front doors share the stage -------------------------------------------------------------------------------------------------
def test_front_doors_share_the_stage(T):
    import sharp_amd

    rng = np.random.default_rng(9)
    centres = rng.normal(0, 3, size=(5, 40))
    X = centres[rng.integers(0, 5, 1500)] + 0.4 * rng.normal(size=(1500, 40)) + 2.0
    Xp = T._prepare(X, pca=True, initial_dims=10, normalize=False)
    assert Xp.shape == (1500, 10)
    idx, dist = T.knn(Xp, 14)
    for name, r in (("umap", sharp_amd.umap(X, n_neighbors=15, pca=10, n_epochs=3, ret_nn=True)),
                    ("snn", sharp_amd.snn(X, k_param=15, pca=10, ret_nn=True)),
                    ("louvain", sharp_amd.louvain(X, n_neighbors=15, pca=10, ret_nn=True))):
        assert np.array_equal(r["nn"]["index"], idx), name
        _same(f"front door {name}: distances", r["nn"]["distance"], dist)
    kw = dict(perplexity=10, max_iter=10, check_duplicates=False)
    a = sharp_amd.Rtsne(X, initial_dims=10, **kw)
    b = sharp_amd.Rtsne(T._prepare(X, pca=True, initial_dims=10, normalize=True), pca=False, normalize=False, **kw)
    _same("front door Rtsne", a["Y"], b["Y"])
