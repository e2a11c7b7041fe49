"""The batch integration on the GPU (csrc/harmony.hip) against tests/_harmony_ref.py: the three stage entries against the
reference's longdouble sums, then whole calls on the planted inputs.

The stage tolerances are bounds on the stage's own roundings, per entry, with u = 2^-53.  None is a tuned number.

assign.  Zhat and Y hold unit rows, so sum |Y_kc Zhat_ic| <= 1 and the fma chain of d terms leaves |dot - exact| <= (d + 1) u.
  D = 2 (1 - dot): one more rounding of a value <= 2, so dD = 2 (d + 3) u, and the minimum over k is within the same.
  x = -(D - min) / sigma: the two D's errors, the subtraction's and the division's roundings: dx = 2 dD / sigma + 2 u |x|.
  e = exp(x) (at most 3 ulp = 6 u as OpenCL bounds it), times the given P (u): relative rho_k = dx_k + 7 u.
  s = the K-term sum of the e_k: relative sum_k R_k rho_k + K u.  R_k = e_k / s (u): |R - exact| <= R_k (rho_k + sum_j R_j rho_j + (K + 8) u),
  plus 1e-300 where exp has left the normal range.
  argmax: the reference's choice, on inputs whose best and second cosine differ by more than 1e6 (d + 1) u (asserted).
sums.  Every entry is a sum of N products (N the cells of the batch, or of the segment for O): whatever the order of the slabs and of the
  fold, |sum - exact| <= (N + 8) u sum |terms|, as DESIGN.md §21 takes it.
correct.  Z_ic - sum_k R_ik W_kc: (K + 8) u (|Z_ic| + sum_k |R_ik W_kc|).

The whole calls compare with the reference's longdouble evaluation within 100 x its recorded rounding spread (_harmony_ref.SPREAD, measured
again by tests/test_harmony_cpu.py), and take its stop decisions, which no rounding reaches (the margins are asserted there)."""
import numpy as np
import pytest

import _harmony_ref as hr

pytestmark = pytest.mark.gpu
U = hr.U


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def hm(sa):
    from sharp_amd import harmony

    return harmony


def unit(rng, n, d):
    X = rng.normal(size=(n, d))
    return X / np.sqrt((X * X).sum(axis=1, keepdims=True))


def clustered(rng, n, d, K, noise=0.3):
    """unit rows around K unit centres, the centres, the labels"""
    Y = unit(rng, K, d)
    lab = rng.integers(0, K, n)
    X = Y[lab] + noise * rng.normal(size=(n, d)) / np.sqrt(d)
    return X / np.sqrt((X * X).sum(axis=1, keepdims=True)), Y, lab


def batches(rng, n, B):
    b = rng.integers(0, B, n)
    b[:B] = np.arange(B)                                                        # every code present
    return b


def assign_tol(Zh, Y, batch, P, sigma, R):
    d, K = Zh.shape[1], Y.shape[0]
    D = 2 * (1 - hr.cosines(Zh, Y))
    x = np.abs((D - D.min(axis=1, keepdims=True)) / sigma).astype(np.float64)
    rho = 2 * 2 * (d + 3) * U / sigma + 2 * U * x + 7 * U
    R = np.asarray(R, np.float64)
    return R * (rho + (R * rho).sum(axis=1, keepdims=True) + (K + 8) * U) + 1e-300


def check_assign(hm, Zh, Y, batch, P, sigma, **kw):
    want = hr.assign(Zh, Y, batch, P, sigma)
    got = hm._assign(Zh, Y, batch, P, sigma, **kw)
    tol = assign_tol(Zh, Y, batch, P, sigma, want)
    i0, i1 = kw.get("i0", 0), kw.get("i1", len(Zh))
    err = np.abs(got[i0:i1] - want[i0:i1].astype(np.float64))
    worst = float((err / tol[i0:i1]).max()) if i1 > i0 else 0.0
    print(f"assign n={len(Zh)} d={Zh.shape[1]} K={len(Y)} sigma={sigma}: max err {err.max() if err.size else 0:.2e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0
    return got, want


# d = 2, 50, 64, 65, 128; K = 2, 63, 64, 65, 100, 256, and K = 256 with d = 128 (Y tiled over clusters); B = 2, 3, 64, 65; an n beyond one
# pass of the grid, untiled and tiled
ASSIGN = [(301, 2, 2, 2), (301, 50, 63, 3), (301, 64, 64, 64), (301, 65, 65, 65), (301, 128, 100, 3), (301, 10, 256, 2), (261, 128, 256, 3),
          (20011, 10, 5, 3), (13007, 128, 65, 2)]


@pytest.mark.parametrize("n,d,K,B", ASSIGN)
def test_assign_against_the_reference(hm, n, d, K, B):
    rng = np.random.default_rng(n + d + K)
    Zh, Y, _ = clustered(rng, n, d, K)
    batch = batches(rng, n, B)
    P = rng.uniform(0.2, 3.0, (B, K))
    check_assign(hm, Zh, Y, batch, P, 0.1)
    if n < 1000:
        check_assign(hm, Zh, Y, batch, None, 0.1)                               # theta = 0 / the first R: no table
        check_assign(hm, Zh, Y, batch, np.ones((B, K)), 0.1)


@pytest.mark.parametrize("n,d,K,B", [c for c in ASSIGN if c[0] < 1000 or c[1] == 10])
def test_argmax_against_the_reference(hm, n, d, K, B):
    rng = np.random.default_rng(7 * n + d + K)
    Zh, Y, _ = clustered(rng, n, d, K)
    cs = np.sort(hr.cosines(Zh, Y), axis=1)
    assert float((cs[:, -1] - cs[:, -2]).min()) > 1e6 * (d + 1) * U             # the premise: no choice within reach of rounding
    a = hm._assign(Zh, Y, batch=batches(rng, n, B), argmax=True)
    assert np.array_equal(a, hr.cosines(Zh, Y).argmax(axis=1))


def test_argmax_ties_go_to_the_lower_cluster(hm):
    rng = np.random.default_rng(5)
    Zh, Y, _ = clustered(rng, 90, 7, 70)
    Y[66] = Y[3]                                                                # two identical centroids, in different lanes' slots
    Y[69] = Y[68]
    a = hm._assign(Zh, Y, batch=batches(rng, 90, 2), argmax=True)
    want = hr.cosines(Zh, Y).argmax(axis=1)
    assert np.array_equal(a, want) and not np.isin(a, (66, 69)).any() and np.isin(a, (3, 68)).any()


@pytest.mark.parametrize("i0,i1", [(0, 1), (5, 68), (3, 67), (0, 65), (40, 40), (199, 200)])
def test_assign_over_a_range_leaves_the_other_rows(hm, i0, i1):
    """blocks of 1, 63, 64 and 65 cells (and none)"""
    rng = np.random.default_rng(11)
    n, d, K, B = 200, 9, 6, 3
    Zh, Y, _ = clustered(rng, n, d, K)
    batch = batches(rng, n, B)
    P = rng.uniform(0.5, 2.0, (B, K))
    mark = rng.uniform(size=(n, K))
    got, _ = check_assign(hm, Zh, Y, batch, P, 0.1, i0=i0, i1=i1, out=mark)
    keep = np.ones(n, bool)
    keep[i0:i1] = False
    assert np.array_equal(got[keep], mark[keep])
    whole = hm._assign(Zh, Y, batch, P, 0.1)
    assert np.array_equal(got[i0:i1], whole[i0:i1])                             # a cell's row does not depend on the range it came in


@pytest.mark.parametrize("sigma", [0.01, 0.002])
def test_assign_on_separated_input(hm, sigma):
    """sigma = 0.01 on separated input; at 0.002 the far clusters' exponentials underflow and R holds exact zeros"""
    rng = np.random.default_rng(13)
    n, d, K, B = 150, 8, 6, 2
    Y = np.eye(K, d)
    lab = rng.integers(0, K, n)
    Zh = Y[lab] + 0.02 * rng.normal(size=(n, d))
    Zh /= np.sqrt((Zh * Zh).sum(axis=1, keepdims=True))
    batch = batches(rng, n, B)
    got, want = check_assign(hm, Zh, Y, batch, rng.uniform(0.5, 2.0, (B, K)), sigma)
    assert np.array_equal(got.argmax(axis=1), lab)
    if sigma == 0.002:
        want64 = want.astype(np.float64)                                        # (longdouble's range holds what underflows in fp64)
        assert (want64 == 0).any() and np.array_equal(got == 0, want64 == 0)
    assert np.abs(got.astype(np.longdouble).sum(axis=1) - 1).max() <= K * 2.0 ** -52


def segments_case(hm, seed=1):
    """n_blocks = 2, B = 3: the segments of batches 0 and 1 hold slab - 1, slab, slab + 1 and 2 slab + 1 cells, batch 2 takes the rest"""
    slab = hm._caps()[0]
    n = 8 * slab
    blk = hr.blocks_of(seed, n, 2)
    batch = np.full(n, 2)
    for j, (c0, c1) in enumerate(((slab - 1, slab), (slab + 1, 2 * slab + 1))):
        at = np.flatnonzero(blk == j)
        assert at.size > c0 + c1
        batch[at[:c0]] = 0
        batch[at[c0:c0 + c1]] = 1
    cnt = [[int(((blk == j) & (batch == b)).sum()) for b in (0, 1)] for j in (0, 1)]
    assert cnt == [[slab - 1, slab], [slab + 1, 2 * slab + 1]]
    return n, batch


SUMS = {"n7_empty_blocks": (7, 2, 2, 2, 20), "single_cell_batch": (90, 5, 4, 3, 4), "B64": (700, 5, 3, 64, 4), "B65": (700, 5, 3, 65, 4),
        "K256_d128": (300, 128, 256, 2, 3), "K100_d50": (900, 50, 100, 3, 20), "K65_d65": (400, 65, 65, 2, 1), "segments": None}


@pytest.mark.parametrize("name", list(SUMS))
def test_sums_against_the_reference(hm, name):
    rng = np.random.default_rng(len(name))
    if name == "segments":
        n, batch = segments_case(hm)
        d, K, B, nb = 6, 5, 3, 2
    else:
        n, d, K, B, nb = SUMS[name]
        batch = batches(rng, n, B)
        if name == "single_cell_batch":
            batch = np.where(batch == 2, 0, batch)
            batch[17] = 2
            assert (batch == 2).sum() == 1
    R = rng.dirichlet(np.ones(K), n)
    if name == "K100_d50":
        R[rng.uniform(size=R.shape) < 0.5] = 0.0                                # exact zeros among the terms
    X = rng.normal(size=(n, d)) * 3.0
    O, S = hm._sums(R, X, batch, B, seed=1, n_blocks=nb)
    Or, Sr, Oa, Sa, On, Sn = hr.sums(R, X, batch, B, 1, nb)
    if name in ("n7_empty_blocks", "B64", "B65"):
        assert (On == 0).any() and (O[On == 0] == 0).all()                      # empty blocks / empty (block, batch) segments
    eo = np.abs(O - Or.astype(np.float64))
    to = ((On + 8) * U)[:, :, None] * Oa.astype(np.float64)
    es = np.abs(S - Sr.astype(np.float64))
    ts = ((Sn + 8) * U)[:, None, None] * Sa.astype(np.float64)
    print(f"sums {name}: O max err {eo.max():.2e} (worst err / bound {(eo / np.maximum(to, 1e-300)).max():.3f}), S {es.max():.2e} "
          f"({(es / np.maximum(ts, 1e-300)).max():.3f})")
    assert (eo <= to).all() and (es <= ts).all()
    O2, S2 = hm._sums(R, X, batch, B, seed=1, n_blocks=nb)
    assert O.tobytes() == O2.tobytes() and S.tobytes() == S2.tobytes()


@pytest.mark.parametrize("n,d,K,B", [(7, 2, 2, 2), (203, 50, 100, 3), (203, 64, 63, 64), (203, 65, 65, 65), (261, 128, 256, 2)])
def test_correct_against_the_reference(hm, n, d, K, B):
    rng = np.random.default_rng(n + d)
    Z = rng.normal(size=(n, d)) * 4.0
    R = rng.dirichlet(np.ones(K), n)
    W = rng.normal(size=(B, K, d))
    batch = batches(rng, n, B)
    got = hm._correct(Z, R, batch, W)
    want = hr.correct(Z, R, batch, W)
    tol = (K + 8) * U * hr.correct_abs(Z, R, batch, W)
    err = np.abs(got - want.astype(np.float64))
    print(f"correct n={n} d={d} K={K}: max err {err.max():.2e}, worst err / bound {(err / tol).max():.3f}")
    assert (err <= tol).all()


def test_ridge_with_an_empty_cluster_then_correct(hm):
    """the library's own W from sums in which one cluster has no mass (s = 0: W_k = 0) and a batch is absent from another, then the
    correction with it, against the reference's W and correction"""
    rng = np.random.default_rng(21)
    n, d, K, B = 203, 9, 6, 3
    Z = rng.normal(size=(n, d)) * 4.0
    R = rng.dirichlet(np.ones(K), n)
    R[:, 4] = 0.0                                                               # nobody joined cluster 4
    batch = batches(rng, n, B)
    R[batch == 1, 2] = 0.0
    R /= R.sum(axis=1, keepdims=True)
    O, S = hm._sums(R, Z, batch, B, seed=1, n_blocks=5)
    N = O.sum(axis=0)
    assert (N[:, 4] == 0).all() and N[1, 2] == 0
    W = hm._ridge(N, S, 1.0)
    want_W = hr.ridge(N.astype(np.longdouble), S.astype(np.longdouble), 1.0)
    assert np.isfinite(W).all() and (W[:, 4] == 0).all()
    assert np.abs(W - want_W.astype(np.float64)).max() <= (B + 8) * U * 4 * np.abs(Z).max()      # |S / N| <= max |Z|: four such terms an entry
    got = hm._correct(Z, R, batch, W)
    want = hr.correct(Z, R, batch, W)
    assert (np.abs(got - want.astype(np.float64)) <= (K + 8) * U * hr.correct_abs(Z, R, batch, W)).all() and np.isfinite(got).all()


def test_workspaces_beyond_the_free_memory_are_refused(sa):
    """the widest tables on many small segments: 1.2 million cells over 4096 batches and 1024 blocks are about as many slabs, each with a
    256 x 128 product of its own -- some 320 GB, beyond the card.  Refused by name before anything is allocated: the device's free memory
    is what it was."""
    import torch

    n, d = 1_200_000, 128
    Z = np.ones((n, d))
    batch = np.arange(n) % 4096
    free0 = torch.cuda.mem_get_info(0)[0]
    with pytest.raises(sa.SharpError, match=r"harmony_integrate: the workspaces need about \d+ MB; the device has \d+ MB free"):
        sa.harmony_integrate(Z, batch, n_clusters=256, n_blocks=1024)
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free1 >= free0 - (1 << 30), (free0, free1)                           # (others may use the card: a gigabyte of slack, against 320)


# ---- whole calls -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    out = {}
    for n in hr.WHOLE:
        Z, b, lab = hr.planted(n)
        out[n] = {"data": (Z, b, lab), "fixed": hr.harmony(Z, b, dt=np.longdouble, **hr.FIXED), "default": hr.harmony(Z, b, dt=np.longdouble)}
    return out


@pytest.mark.parametrize("n", hr.WHOLE)
def test_fixed_counts_against_the_reference(sa, planted, n):
    Z, b, _ = planted[n]["data"]
    want = planted[n]["fixed"]
    got = sa.harmony_integrate(Z, b, ret_R=True, **hr.FIXED)
    assert got["n_iter"] == 5 and list(got["rounds"]) == [10] * 5 and not got["converged"] and got["n_clusters"] == want["n_clusters"]
    for key, rel in (("Z_corr", True), ("Y", False), ("R", False)):
        e = hr.spread(got[key], want[key], rel)
        print(f"planted({n}) fixed counts, {key}: {e:.2e} against 100 x {hr.SPREAD[n][key]:.1e}")
        assert e <= 100 * hr.SPREAD[n][key]
    assert np.abs(got["R"].astype(np.longdouble).sum(axis=1) - 1).max() <= got["n_clusters"] * 2.0 ** -52
    again = sa.harmony_integrate(Z, b, ret_R=True, **hr.FIXED)
    for key in ("Z_corr", "Y", "R", "objective"):
        assert got[key].tobytes() == again[key].tobytes(), key


@pytest.mark.parametrize("n", hr.WHOLE)
def test_defaults_take_the_reference_decisions(sa, planted, n):
    Z, b, lab = planted[n]["data"]
    want = planted[n]["default"]
    got = sa.harmony_integrate(Z, b)
    dec = hr.DECISIONS[n]
    assert (want["n_iter"], tuple(want["rounds"]), want["converged"]) == (dec["n_iter"], dec["rounds"], dec["converged"])
    assert (got["n_iter"], tuple(got["rounds"]), got["converged"]) == (dec["n_iter"], dec["rounds"], dec["converged"])
    e = hr.spread(got["objective"], want["objective"])
    print(f"planted({n}) defaults: objective {got['objective']}, off by {e:.2e} against 100 x {hr.SPREAD[n]['objective']:.1e}")
    assert e <= 100 * hr.SPREAD[n]["objective"]
    sb, sl, _ = hr.neighbour_shares(got["Z_corr"], b, lab)
    q = hr.QUALITY[n]
    print(f"planted({n}) defaults: same batch {sb:.4f}, same label {sl:.5f}")
    assert sb <= q["same_batch_worst"] + q["same_batch_spread"] and sl >= q["same_label_worst"] - q["same_label_spread"]
    assert got["n_batches"] == 3 and list(got["batch_levels"]) == [0, 1, 2] and "R" not in got
    # labels of any kind
    names = np.array(["run-c", "run-a", "run-b"])[b]
    got2 = sa.harmony_integrate(Z, names)
    perm = np.array([2, 0, 1])[b]                                               # the codes np.unique gives these names
    got3 = sa.harmony_integrate(Z, perm)
    assert list(got2["batch_levels"]) == ["run-a", "run-b", "run-c"] and got2["Z_corr"].tobytes() == got3["Z_corr"].tobytes()


def separated(n=240, seed=3):
    """six well separated clusters in d = 8, two batches with an offset; cluster 5 lives in batch 1 alone"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 6, n)
    b = rng.integers(0, 2, n)
    b[lab == 5] = 1
    off = np.zeros((2, 8))
    off[1, 6] = 1.0
    Z = 8.0 * np.eye(6, 8)[lab] + off[b] + 0.2 * rng.normal(size=(n, 8))
    return Z, b, lab


def test_exact_zeros_and_an_empty_start_cluster(sa):
    """sigma = 0.002: R holds exact zeros (the R log R rule) and clusters without mass in a batch, and -- two start cells made identical,
    found by the hash -- a start cluster that stays empty through the Lloyd rounds and keeps its Y.  Fixed counts; the bound is 100 x the
    reference's own spread (fp64 against longdouble) on this input, measured here.  (The W = 0 rule of a cluster with s = 0 is
    tested on the library's own ridge: test_ridge_with_an_empty_cluster_then_correct, tests/test_harmony_cpu.py.)"""
    Z, b, _ = separated()
    n, K, seed = len(Z), 8, 1
    st = hr.start_cells(seed, n, K)                                             # found by the hash
    Z[st[5]] = Z[st[2]]
    kw = dict(n_clusters=K, sigma=0.002, max_iter=3, max_iter_cluster=4, epsilon_cluster=0.0, epsilon_harmony=0.0, n_blocks=5, seed=seed)
    ld = hr.harmony(Z, b, dt=np.longdouble, **kw)
    f64 = hr.harmony(Z, b, **kw)
    assert (f64["R"] == 0).any() and f64["start_empty"][-1] >= 1 and ld["start_empty"] == f64["start_empty"]
    assert ld["cos_gap"][0] == 0 and min(ld["cos_gap_positive"]) > 1e6 * 2 * 9 * U      # the planted tie is exact; nothing else is near one
    got = sa.harmony_integrate(Z, b, ret_R=True, **kw)
    assert np.array_equal(got["R"] == 0, f64["R"] == 0)
    for key, rel in (("Z_corr", True), ("Y", False), ("R", False), ("objective", True)):
        own = max(hr.spread(f64[key], ld[key], rel), 2 * U)
        e = hr.spread(got[key], ld[key], rel)
        print(f"separated, {key}: {e:.2e} against 100 x {own:.1e}")
        assert e <= 100 * own
    assert np.isfinite(got["objective"]).all()


def test_theta_zero_and_small_inputs(sa):
    """theta = 0 (no penalty: P = 1); n = 7 with 20 blocks (empty blocks); one batch of a single cell"""
    Z, b, _ = separated(120, 4)
    kw = dict(n_clusters=6, theta=0.0, max_iter=2, max_iter_cluster=3, epsilon_cluster=0.0, epsilon_harmony=0.0)
    ld, f64 = hr.harmony(Z, b, dt=np.longdouble, **kw), hr.harmony(Z, b, **kw)
    got = sa.harmony_integrate(Z, b, ret_R=True, **kw)
    for key, rel in (("Z_corr", True), ("R", False)):
        assert hr.spread(got[key], ld[key], rel) <= 100 * max(hr.spread(f64[key], ld[key], rel), 2 * U), key
    Z7 = Z[:7] + 0.0
    b7 = np.array([0, 1, 0, 1, 0, 0, 2])                                        # batch 2: a single cell
    kw = dict(n_clusters=2, max_iter=2, max_iter_cluster=3, epsilon_cluster=0.0, epsilon_harmony=0.0, init_iter=2)
    ld, f64 = hr.harmony(Z7, b7, dt=np.longdouble, **kw), hr.harmony(Z7, b7, **kw)
    got = sa.harmony_integrate(Z7, b7, ret_R=True, **kw)
    for key, rel in (("Z_corr", True), ("R", False)):
        assert hr.spread(got[key], ld[key], rel) <= 100 * max(hr.spread(f64[key], ld[key], rel), 2 * U), key


def test_readme_idiom_end_to_end(sa):
    """expression_pca -> harmony_integrate -> knn -> louvain_snn on two Poisson blocks with a block effect"""
    import scipy.sparse as sp

    rng = np.random.default_rng(0)
    m, per = 300, 180
    prog = rng.gamma(2.0, 1.0, (3, m))
    blocks, labs = [], []
    for q in range(2):
        lab = rng.integers(0, 3, per)
        rate = prog[lab] * (1.0 + (0.8 if q else 0.0) * (np.arange(m) % 2))     # the second block doubles every other gene
        blocks.append(sp.csc_matrix(rng.poisson(rate).T.astype(np.float64)))
        labs.append(lab)
    lab = np.concatenate(labs)
    batch = sa.batch_of_blocks(blocks)
    assert batch.shape == (2 * per,) and (batch[:per] == 0).all() and (batch[per:] == 1).all()
    pc = sa.expression_pca(blocks, 10)
    hz = sa.harmony_integrate(pc["scores"], batch, n_clusters=6)
    before = hr.neighbour_shares(pc["scores"], batch, lab, 15)
    after = hr.neighbour_shares(hz["Z_corr"], batch, lab, 15)
    print(f"idiom: same batch {before[0]:.3f} -> {after[0]:.3f}, same label {before[1]:.3f} -> {after[1]:.3f}")
    assert after[0] < before[0] and after[1] >= before[1] - 0.02
    idx, _ = sa.knn(hz["Z_corr"], 19)
    res = sa.louvain_snn(idx)
    assert res["membership"].shape == (2 * per,) and res["n_communities"] >= 2


def test_every_refusal_by_name(sa, hm):
    Z, b, _ = hr.planted(60)
    bad = Z.copy()
    bad[7] = 0.0
    nan = Z.copy()
    nan[9, 2] = np.nan
    for args, kw, msg in (((bad, b), {}, r"a zero row in Z \(cell 7,"), ((nan, b), {}, "a non-finite value in Z"),
                          ((Z, np.zeros(60, int)), {}, "one batch: nothing to integrate"), ((Z, b), {"n_clusters": 61}, "n_clusters exceeds the number of cells"),
                          ((Z[:, :1], b), {}, "need 2 <= d <= 128 columns"), ((np.ones((60, 129)), b), {}, "need 2 <= d <= 128 columns")):
        with pytest.raises(sa.SharpError, match="harmony_integrate: " + msg):
            sa.harmony_integrate(*args, **kw)
    with pytest.raises(sa.SharpError, match=r"harmony_sums: an empty batch code \(1\)"):
        hm._sums(np.ones((60, 2)), Z, np.where(b == 1, 0, b), 3)
    # the library's own refusals with a device present
    import ctypes as C

    from sharp_amd._lib import f64, i32, lib

    ni, cv = C.c_int(), C.c_int()
    out = [np.zeros((60, 10)), np.zeros((2, 10)), np.zeros(2), np.zeros(2, np.int32)]
    b32 = b.astype(np.int32)
    rc = lib().sharp_harmony(f64(bad), 60, 10, i32(b32), 3, 2, 0.1, 2.0, 1.0, 2, 5, 20, 1e-5, 1e-4, 3, 1, f64(out[0]), f64(out[1]), f64(out[2]),
                             i32(out[3]), C.byref(ni), C.byref(cv), None)
    assert rc != 0 and b"harmony_integrate: a zero row in Z (cell 7," in lib().sharp_last_error()
    rc = lib().sharp_harmony(f64(Z), 60, 10, i32(b32), 4, 2, 0.1, 2.0, 1.0, 2, 5, 20, 1e-5, 1e-4, 3, 1, f64(out[0]), f64(out[1]), f64(out[2]),
                             i32(out[3]), C.byref(ni), C.byref(cv), None)
    assert rc != 0 and b"an empty batch code (3)" in lib().sharp_last_error()
