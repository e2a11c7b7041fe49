"""t-SNE on the MI355X at the shapes where its launches split (csrc/tsne.hip), against tests/_tsne_ref.py and
tests/_tsne_bh_ref.py: the exact repulsion with several tiles per chunk, several chunks and a second row launch; the calibration and
the k-NN lists with three and four 64-wide slots; the k-NN's candidate selection on input far from the origin; the Barnes-Hut layered
sums with a fourth layer; the per-point KL.

Every shape is the smallest that reaches its branch.  The constants that decide this are read from tsne.hip itself (_constants), and
each test asserts from them that its shape still splits the way its comment says, so a later change of a constant fails the test
instead of emptying it."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _tsne_bh_ref as bh
import _tsne_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24   # the unit roundoff of fp32


@pytest.fixture(scope="module")
def T():
    import sharp_amd
    from sharp_amd import tsne

    sharp_amd.init(0)
    return tsne


def _blobs(n, d, groups, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3, size=(groups, d))
    lab = rng.integers(0, groups, n)
    return centres[lab] + spread * rng.normal(size=(n, d)), lab


def _mixture(n, dims, seed, groups=8):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 25, size=(groups, dims))
    return centres[rng.integers(0, groups, n)] + 3 * rng.normal(size=(n, dims))


# ---- the launch arithmetic of tsne.hip, from its own constants ------------------------------------------------------------------------
def _constants():
    src = open(os.path.join(ROOT, "sharp_amd", "csrc", "tsne.hip")).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (pattern, m)
        return m[0]

    return {"RT": int(one(r"constexpr int RT = (\d+);")),
            "pairs": float(one(r"constexpr double kPairsPerLaunch = ([0-9.e+]+);")),
            "wgs": int(one(r"\((\d+) \+ rb - 1\) / rb\)\);\s*// >= ~\d+ workgroups per launch")),
            "radix": int(one(r"constexpr int kBhRadix = (\d+);")),
            "slabs": int(one(r"constexpr int kBhSlabs = (\d+);"))}


def _rep_plan(n, c):
    """rep_plan() of tsne.hip: (rows per launch, columns per chunk, chunks)"""
    RT = c["RT"]
    n_up = -(-n // RT) * RT
    rows = min(n_up, max(RT, int(c["pairs"] / n) // RT * RT))
    rb = -(-rows // RT)
    nc = max(1, min(-(-n // RT), -(-c["wgs"] // rb)))
    cj = -(-(-(-n // nc)) // RT) * RT
    return rows, cj, -(-n // cj)


def _tiles(n, c):
    """the LDS tiles of every column chunk: a list (per chunk) of tile lengths"""
    _, cj, nc = _rep_plan(n, c)
    out = []
    for b in range(nc):
        length = min(n, (b + 1) * cj) - b * cj
        out.append([min(c["RT"], length - t) for t in range(0, length, c["RT"])])
    return out


def _exact_gpu(T, Y):
    """rep and Z of the exact path: one gradient with an empty P is dY = -rep / Z"""
    n = Y.shape[0]
    dY, Z = T._gradient_bh(np.zeros(n + 1, np.int64), np.zeros(1, np.int32), np.zeros(1), Y, 0.0)
    return -dY * Z, Z, dY


def _f32(Y):
    """Y rounded to fp32: the kernel's fp32 copy is then exact and only its arithmetic is under test"""
    return Y.astype(np.float32).astype(np.float64)


def _check_repulsion(tag, rep, Z, rep_ref, Z_ref, A, n):
    """The bound, derived and not tuned: a pair term costs a handful of fp32 roundings, a tile sums at most RT = 256 terms in fp32,
    everything above the tile is fp64.  So |rep_ik - ref| <= (256 + 12) 2^-24 A_ik and |Z - ref| <= (256 + 6) 2^-24 (Z + n) (the
    fp32 row sums hold the self pairs too: sum_i (z_i + 1) = Z + n)."""
    bound = (256 + 12) * U32 * A
    ratio = np.abs(rep - rep_ref) / bound
    zratio = abs(Z - Z_ref) / ((256 + 6) * U32 * (Z_ref + n))
    print(f"{tag}: largest |rep - ref| / bound = {ratio.max():.3e} (row {int(ratio.max(1).argmax())}), |Z - ref| / bound = {zratio:.3e}")
    assert np.isfinite(rep).all() and (A > 0).all()
    assert (ratio <= 1.0).all(), (tag, ratio.max())
    assert zratio <= 1.0, (tag, zratio)


# ---- 2. the exact repulsion at every launch shape --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [1, 2, 3])
@pytest.mark.parametrize("n", [257, 513])
def test_exact_repulsion_one_row_past_a_tile(T, n, dims):
    """RT = 256: n = 257 and 513 are one row past one and two tiles: the last row block holds a single active row, and the column
    chunks are 256 (, 256), 1: one-tile chunks, the last a single point"""
    c = _constants()
    tiles = _tiles(n, c)
    assert _rep_plan(n, c)[0] >= n and len(tiles) == n // c["RT"] + 1 and tiles[-1] == [1]
    Y = _f32(_mixture(n, dims, 300 + dims) * 0.2)
    rep_ref, z_ref, A = ref.exact_repulsion(Y)
    rep, Z, _ = _exact_gpu(T, Y)
    _check_repulsion(f"n={n} dims={dims}", rep, Z, rep_ref, z_ref.sum(), A, n)


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_exact_repulsion_four_tiles_per_chunk(T, dims):
    """n = 20 011: the 2048-workgroup rule gives 79 row blocks, hence 26 -> 20 chunks of 1 024 columns = four tiles of RT = 256 each
    (the tile loop carries its fp64 partials across tiles; the self pair sits in one of the four), and the last chunk is
    256 + 256 + 43 (a short last tile).  One row launch.  (The loop first runs twice at n > ~11 600; 20 011 is odd, prime, and gives
    more than two tiles.)"""
    n = 20011
    c = _constants()
    tiles = _tiles(n, c)
    assert _rep_plan(n, c)[0] >= n                                   # one row launch
    assert len(tiles) > 1 and all(len(t) > 1 for t in tiles)        # several chunks, several tiles in each
    assert tiles[0] == [c["RT"]] * 4 and 0 < tiles[-1][-1] < c["RT"] and len(tiles[-1]) == 3
    Y = _f32(_mixture(n, dims, 310 + dims) * 0.2)   # (in 1-D a few rows coincide after the rounding: pairs at q = 1, as in the kernel)
    rep_ref, z_ref, A = ref.exact_repulsion(Y)
    rep, Z, _ = _exact_gpu(T, Y)
    _check_repulsion(f"n={n} dims={dims}", rep, Z, rep_ref, z_ref.sum(), A, n)


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_exact_repulsion_two_row_launches(T, dims):
    """n = 330 001: kPairsPerLaunch = 1e11 gives 302 848 rows per launch (1 183 blocks of RT = 256), so a second launch runs rows
    302 848 .. 330 000: row0 > 0, `part` rewritten and folded again, the last active block partial (27 153 = 106 * 256 + 17 rows) and
    the rest of its grid idle.  Two column chunks of 645 tiles; the last tile holds 17 points.  The smallest such n is ~316 300; this
    one also ends both the rows and the columns inside a tile.
    The reference is the multiset form: 4 099 positions (a prime; 16 tiles' worth) with multiplicities that sum to
    n, assigned in a shuffled order so that every tile mixes positions.  Every row and Z are checked, and a second call must return
    the same bits."""
    n, m = 330001, 4099
    c = _constants()
    rows, cj, nc = _rep_plan(n, c)
    tiles = _tiles(n, c)
    assert rows < n and n - rows > c["RT"] and (n - rows) % c["RT"] != 0      # a second launch, with a partial last block
    assert nc > 1 and all(len(t) > 1 for t in tiles) and 0 < tiles[-1][-1] < c["RT"]
    rng = np.random.default_rng(320 + dims)
    pos = _f32(_mixture(m, dims, 330 + dims) * 0.2)
    cnt = rng.multinomial(n - m, np.full(m, 1.0 / m)) + 1             # every position at least once
    assign = rng.permutation(np.repeat(np.arange(m), cnt))
    assert cnt.sum() == n and assign.shape == (n,)
    rep_p, z_p, A_p = ref.multiset_repulsion(pos, cnt)
    Y = pos[assign]
    rep, Z, dY = _exact_gpu(T, Y)
    _check_repulsion(f"n={n} dims={dims}", rep, Z, rep_p[assign], float(cnt @ z_p), A_p[assign], n)
    _, Z2, dY2 = _exact_gpu(T, Y)
    assert Z2 == Z and np.array_equal(dY2, dY)                        # bitwise


# ---- 3. calibration and k-NN lists at three and four slots -----------------------------------------------------------------------------
def _clump_input():
    """3 001 x 10, six blobs; rows 100-399 a clump of sigma = 1e-4 around row 100 (more rows than K = 255, so every neighbour of a
    clump row is in the clump and beta doubles some 25 times from 1); row 3000 pushed 40 / sqrt(d) out in every column (far from
    everything: beta halves); row 2999 scaled by 3; normalised as Rtsne does"""
    X, _ = _blobs(3001, 10, 6, 41)
    rng = np.random.default_rng(42)
    X[101:400] = X[100] + 1e-4 * rng.normal(size=(299, 10))
    X[3000] += 40.0 / np.sqrt(10.0)
    X[2999] *= 3.0
    return ref.normalize(X)


@pytest.fixture(scope="module")
def clump():
    X = _clump_input()
    idx, dist = ref.knn(X, 255)
    return X, idx, dist


def test_knn_lists_of_255(T, clump):
    """K = 255, the permitted maximum: the LDS lists of knn_kernel / knn_merge_kernel are four 64-wide strides long (the last of 63)"""
    X, ridx, rdist = clump
    idx, dist = T._knn(X, 255)
    assert np.array_equal(idx, ridx)
    np.testing.assert_allclose(dist, rdist, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("perplexity", [85, 50, 43, 21.5])
def test_calibration_in_every_slot(T, clump, perplexity):
    """calib_kernel holds a row's K distances in 4 x 64 register slots: K = 255 fills four (the last short by one), 150 three (the
    third partly), 129 puts a single entry in the third, 64 fills exactly one.  The clump rows double beta from 1 past 2^32 with the
    upper bound open.  (The two far rows do not halve it: after the normalisation no row of this input does, they stop near 8 and
    64.  test_calibration_halving_with_the_lower_bound_open has that branch.)
    The comparison is exact in the structure and 1e-10 in the values, which holds only if the kernel takes the reference's bisection
    steps; so the reference's own stop decisions must not hang on rounding: every row stops before step 200 and never comes closer
    than 1e-12 to the tolerance (H carries an error of a few 1e-16 log K)."""
    X, ridx, rdist = clump
    K = int(np.floor(3 * perplexity))
    assert K == {85: 255, 50: 150, 43: 129, 21.5: 64}[perplexity] and (K + 63) // 64 == {255: 4, 150: 3, 129: 3, 64: 1}[K]
    Pc, steps, margin = ref.calibrate(rdist[:, :K], perplexity, return_trace=True)
    print(f"K={K}: most steps {steps.max()}, smallest margin {margin.min():.3e}")
    assert steps.max() < 200 and margin.min() >= 1e-12
    beta = np.log(Pc[:, 0] / Pc[:, K - 1]) / (rdist[:, K - 1] - rdist[:, 0])
    assert beta[100:400].min() > 2.0 ** 24                           # long doubling
    rp, col, val = T._affinities(X, perplexity)
    P = ref.joint_p(X, perplexity)
    assert np.array_equal(rp, P.indptr) and np.array_equal(col, P.indices)
    np.testing.assert_allclose(val, P.data, rtol=1e-10, atol=0)


def test_calibration_halving_with_the_lower_bound_open(T):
    """The other open-bound branch: prepared input on a scale of tens (sharp_tsne_affinities takes it as it is; so does
    Rtsne(normalize=False)) has squared distances in the hundreds, and every row halves beta from 1 several times before the lower
    bound closes.  K = 129: three slots, the third holding one entry.  The reference's margins are asserted as above."""
    X, _ = _blobs(700, 10, 3, 45)
    X = X * 20.0
    perplexity, K = 43, 129
    _, dist = ref.knn(X, K)
    Pc, steps, margin = ref.calibrate(dist, perplexity, return_trace=True)
    print(f"halving: most steps {steps.max()}, smallest margin {margin.min():.3e}")
    assert steps.max() < 200 and margin.min() >= 1e-12
    beta = np.log(Pc[:, 0] / Pc[:, K - 1]) / (dist[:, K - 1] - dist[:, 0])
    assert beta.max() < 2.0 ** -4                                      # every row halves at least five times
    rp, col, val = T._affinities(X, perplexity)
    P = ref.joint_p(X, perplexity)
    assert np.array_equal(rp, P.indptr) and np.array_equal(col, P.indices)
    np.testing.assert_allclose(val, P.data, rtol=1e-10, atol=0)


# ---- 4. the k-NN on translated input ---------------------------------------------------------------------------------------------------
def _translated_input(c):
    """1 500 x 10, six blobs, rows 100-399 a clump of sigma = 1e-3, every value shifted by c"""
    X, _ = _blobs(1500, 10, 6, 51)
    rng = np.random.default_rng(52)
    X[101:400] = X[100] + 1e-3 * rng.normal(size=(299, 10))
    return X + c


@pytest.fixture(scope="module", params=[0.0, 1e3, 1e4])
def translated(request):
    X = _translated_input(request.param)
    idx, dist = ref.knn(X, 256)
    return request.param, X, idx, dist


@pytest.mark.parametrize("K", [90, 255])
def test_knn_on_translated_input(T, translated, K):
    """Distances do not depend on a translation, but the form ||x_i||^2 + ||x_j||^2 - 2 x_i.x_j that selects the candidates loses
    eps ||x||^2 to cancellation: at c = 1e4 that is ~1e-6, the squared distances inside the clump are ~2e-5 and 300 of them lie that
    close together.  tsne_knn therefore selects on centred coordinates w = x - mean.
    Premise, asserted on the reference: every row's gap between its K-th and (K + 1)-th distance exceeds 2 B,
    B = 4 (d + 4) 2^-53 (||w_i||^2 + max ||w||^2), so that any selection whose error stays within B of the centred form is exact."""
    c, X, ridx, rdist = translated
    n, d = X.shape
    w2 = ((X - X.mean(0)) ** 2).sum(1)
    B = 4 * (d + 4) * 2.0 ** -53 * (w2 + w2.max())
    gap = rdist[:, K] - rdist[:, K - 1]
    print(f"c={c:g} K={K}: smallest gap / B = {(gap / B).min():.1f}")
    assert (gap > 2 * B).all()
    idx, dist = T._knn(X, K)
    wrong = np.flatnonzero((np.sort(idx, 1) != np.sort(ridx[:, :K], 1)).any(1))
    assert wrong.size == 0, f"c={c:g} K={K}: {wrong.size} rows with a wrong neighbour set, the first {wrong[:5]}"
    assert np.array_equal(idx, ridx[:, :K])
    np.testing.assert_allclose(dist, rdist[:, :K], rtol=1e-12, atol=1e-300)
    # the same through the affinities Rtsne(pca=False, normalize=False) builds from them: the pattern of P is the neighbour sets
    # and their transposes
    rp, col, _ = T._affinities(X, K / 3.0)
    M = sp.csr_matrix((np.ones(n * K), (np.repeat(np.arange(n), K), ridx[:, :K].ravel())), shape=(n, n))
    S = (M + M.T).tocsr()
    S.sort_indices()
    assert np.array_equal(rp, S.indptr) and np.array_equal(col, S.indices)


@pytest.mark.parametrize("K", [90, 255])
@pytest.mark.parametrize("c", [0.0, 1e3, 1e4])
def test_rtsne_on_translated_input(T, c, K):
    """Rtsne(pca=False, normalize=False) hands the caller's values to the k-NN as they are: one iteration against the reference
    run, through the per-point KL (a row with another neighbour set has another row of P and another cost).  Bounds: those of
    test_ten_iterations_from_y_init, the one on the KL taken of the largest entry."""
    import sharp_amd

    X = _translated_input(c)
    perplexity = K / 3.0
    Y0 = np.random.default_rng(53).normal(size=(X.shape[0], 2)) * 1e-2
    _, dist = ref.knn(X, K)
    _, steps, margin = ref.calibrate(dist, perplexity, return_trace=True)
    assert steps.max() < 200 and margin.min() >= 1e-12
    out = sharp_amd.Rtsne(X, perplexity=perplexity, pca=False, normalize=False, check_duplicates=False, max_iter=1, Y_init=Y0)
    P = ref.joint_p(X, perplexity)
    Yr, _ = ref.optimise(P, Y0, max_iter=1, stop_lying_iter=0, mom_switch_iter=0)
    costs = ref.kl(P, Yr, per_point=True)
    np.testing.assert_allclose(out["Y"], Yr, rtol=0, atol=1e-6 * np.abs(Yr).max())
    np.testing.assert_allclose(out["costs"], costs, rtol=0, atol=1e-5 * costs.max())


# ---- 5. Barnes-Hut with a fourth layer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [0.25, 0.5, 0.8])
@pytest.mark.parametrize("dims", [2, 3])
def test_barnes_hut_four_layers(T, dims, theta):
    """kBhRadix = 32: the centres of mass come from layered sums of lengths 40 000, 1 250, 40 and 2; a fourth layer needs
    n > 32^3 = 32 768, and 40 000 makes the top two layers end in partial chunks (40 = 32 + 8).  The bounding box takes 156 slabs of
    257 rows (the last shorter)."""
    n = 40000
    c = _constants()
    lens = [n]
    while lens[-1] > c["radix"]:
        lens.append(-(-lens[-1] // c["radix"]))
    assert lens == [40000, 1250, 40, 2]
    nslab = min(c["slabs"], max(1, n // 256))
    assert -(-n // -(-n // nslab)) == 156
    Y = _mixture(n, dims, 340 + dims) * 0.2
    Y[[11, 1200, 39000]] = Y[3]                       # exact duplicates: one leaf
    Y[500] = Y[501]
    P = sp.csr_matrix((n, n))
    g, Z = T._gradient_bh(np.zeros(n + 1, np.int64), np.zeros(1, np.int32), np.zeros(1), Y, theta)
    gr, Zr = bh.bh_gradient(P, Y, theta, return_z=True)
    np.testing.assert_allclose(Z, Zr, rtol=1e-6)
    np.testing.assert_allclose(g, gr, rtol=0, atol=1e-5 * np.abs(gr).max())


# ---- 6. the per-point KL ---------------------------------------------------------------------------------------------------------------
def test_per_point_costs_after_ten_iterations(T):
    """test_tsne_gpu.py's ten-iteration run, with `costs` (kl_kernel's per-row output) compared row by row instead of as a sum; the
    bound is that test's 1e-5 on the sum (set by the fp32 Z), taken of the largest entry"""
    import sharp_amd

    X, _ = _blobs(1200, 20, 4, 15)
    Y0 = np.random.default_rng(16).normal(size=(1200, 2)) * 1e-2
    out = sharp_amd.Rtsne(X, perplexity=20, max_iter=10, Y_init=Y0, stop_lying_iter=5, mom_switch_iter=5)
    P = ref.joint_p(ref.prepare(X, True, 50), 20)
    Yr, cr = ref.optimise(P, Y0, max_iter=10, stop_lying_iter=5, mom_switch_iter=5)
    costs = ref.kl(P, Yr, per_point=True)
    np.testing.assert_allclose(costs.sum(), cr[-1], rtol=1e-12)
    assert out["costs"].shape == (1200,)
    np.testing.assert_allclose(out["costs"], costs, rtol=0, atol=1e-5 * costs.max())
