"""The batch integration (tests/_harmony_ref.py) on the CPU: the hash and the working order against Python integers, the
closed-form ridge correction against numpy.linalg.solve, the fold-the-others O tables against a direct sum, the symmetric input that the
correction must leave alone, what the reference achieves on the planted inputs, its own rounding spread (from which the GPU tolerances
of the whole calls are taken), the premises of the GPU cases, and the refusals that need no device.

Figures of the reference (printed by the tests).  planted(1500), K = 50, seeds 1 .. 5: the share of a cell's 30 nearest neighbours in its
own batch 0.672 before, 0.3806 .. 0.3816 after (0.336 is chance); the same-label share 0.9983 before, 0.99976 .. 0.99978 after, every
cluster >= 0.9990; three outer iterations, converged, (20, 10, 2) rounds at seed 1.  planted(1025), K = 34: 0.652 -> 0.3672 .. 0.3694,
same label >= 0.99954; (18, 3, 2) rounds.  Rounding spread (fp64 against longdouble, cells summed in the stored and in the working order),
fixed counts: Z_corr 1.1e-15 / 1.6e-15 of max |Z_corr|, Y 7.4e-16 / 8.5e-16, R 1.7e-15 / 3.5e-15; the objective of the default call
2.5e-13 / 8.2e-14 absolute.  Smallest stop margin 3.0e-5 / 7.8e-5: 1e8 and 9e8 times the objective's spread.  Smallest gap between the best
and the second cosine of a start round 3.9e-6 / 1.5e-5 against a dot bound of 2.4e-15."""
import ctypes as C

import numpy as np
import pytest

import _harmony_ref as hr


@pytest.fixture(scope="module")
def whole():
    """per whole-call input: the data, the default call over the seeds (fp64), and the three evaluations of the fixed and default calls"""
    out = {}
    for n in hr.WHOLE:
        Z, b, lab = hr.planted(n)
        out[n] = {"data": (Z, b, lab), "seeds": [hr.harmony(Z, b, seed=s) for s in hr.SEEDS],
                  "fixed": [hr.harmony(Z, b, **hr.FIXED), hr.harmony(Z, b, cells="working", **hr.FIXED), hr.harmony(Z, b, dt=np.longdouble, **hr.FIXED)],
                  "default": [hr.harmony(Z, b), hr.harmony(Z, b, cells="working"), hr.harmony(Z, b, dt=np.longdouble)]}
    return out


def test_hash_bits_against_python_integers():
    assert hr.mix64(0) == 0 and hr.mix64(1) == 0x5692161D100B05E5            # splitmix64's finaliser
    for seed in (0, 1, 7, 2 ** 40 + 3):
        for s in (0, 1):
            want = [hr.mix64(hr.mix64((seed * hr.G + s) & hr.M64) + i) for i in range(300)]
            assert hr.h(seed, s, 300).tolist() == want
    assert hr.blocks_of(1, 300, 20).tolist() == [hr.mix64(hr.mix64(hr.G & hr.M64) + i) % 20 for i in range(300)]


def test_working_order_and_start_cells():
    rng = np.random.default_rng(0)
    n, B, nb = 500, 3, 20
    batch = rng.integers(0, B, n)
    order = hr.working_order(batch, 1, nb)
    blk = hr.blocks_of(1, n, nb)
    keys = [(int(blk[i]), int(batch[i]), int(i)) for i in order]
    assert keys == sorted(keys) and sorted(order.tolist()) == list(range(n))
    # every (block, batch) segment is contiguous
    seg = blk[order] * B + batch[order]
    assert (np.diff(seg) >= 0).all()
    hv = hr.h(1, 1, n)
    st = hr.start_cells(1, n, 17)
    assert st.tolist() == sorted(range(n), key=lambda i: (int(hv[i]), i))[:17]
    # n = 7 over 20 blocks: blocks stay empty
    assert len(set(hr.blocks_of(1, 7, 20).tolist())) < 20


def test_closed_form_ridge_against_solve():
    rng = np.random.default_rng(1)
    B, K, d, lam = 5, 7, 4, 1.0
    N = rng.uniform(0.0, 30.0, (B, K))
    N[2, 3] = 0.0                                                              # a batch absent from a cluster
    S = rng.normal(size=(B, K, d)) * N[:, :, None]
    W = hr.ridge(N, S, lam)
    Ws = hr.ridge_solve(N, S, lam)
    # the system's condition is at most (max N + lam) / (lam min q): a relative 1e-10 is far above both roundings
    assert np.abs(W - Ws).max() <= 1e-10 * np.abs(Ws).max()
    # a cluster without mass: s = 0, W = 0
    N[:, 1] = 0.0
    S[:, 1] = 0.0
    assert (hr.ridge(N, S, lam)[:, 1] == 0).all()


def test_the_library_ridge_against_the_reference():
    """sharp_harmony_ridge is the host function the whole call runs between its sums and its correction; it needs no device"""
    from sharp_amd import harmony

    rng = np.random.default_rng(4)
    B, K, d, lam = 5, 7, 4, 1.0
    N = rng.uniform(0.0, 30.0, (B, K))
    N[2, 3] = 0.0                                                              # a batch absent from a cluster
    N[:, 1] = 0.0                                                              # a cluster without mass: s = 0
    S = rng.normal(size=(B, K, d)) * N[:, :, None]
    W = harmony._ridge(N, S, lam)
    want = hr.ridge(N.astype(np.longdouble), S.astype(np.longdouble), lam)
    assert np.isfinite(W).all() and (W[:, 1] == 0).all() and (want[:, 1] == 0).all()
    # per entry: num and s are folds of B terms, then three operations: (B + 8) u on every term's magnitude
    q = N / (N + lam)
    mag = (np.abs(S) + N[:, :, None] * ((np.abs(S) * (1 + q[:, :, None])).sum(axis=0) / np.maximum(lam * q.sum(axis=0), 1e-300)[:, None])[None]) \
        / (N + lam)[:, :, None]
    err = np.abs(W - want.astype(np.float64))
    print(f"library ridge: max err {err.max():.2e}, worst err / bound {(err / np.maximum((B + 8) * hr.U * mag, 1e-300)).max():.3f}")
    assert (err <= (B + 8) * hr.U * mag).all()
    live = np.arange(K) != 1
    Ws = hr.ridge_solve(N[:, live], S[:, live], lam)
    assert np.abs(W[:, live] - Ws).max() <= 1e-10 * np.abs(Ws).max()
    # every cluster empty: W = 0, not NaN
    assert (harmony._ridge(np.zeros((2, 2)), np.zeros((2, 2, 3)), 0.5) == 0).all()
    with pytest.raises(harmony.SharpError, match="harmony_ridge: lam must be > 0"):
        harmony._ridge(N, S, 0.0)


def test_fold_the_others_against_a_direct_sum():
    rng = np.random.default_rng(2)
    n, K, B, nb = 400, 5, 3, 20
    R = rng.dirichlet(np.ones(K), n)
    batch = rng.integers(0, B, n)
    O = hr.sums(R, rng.normal(size=(n, 3)), batch, B, 1, nb)[0]               # nb x B x K
    blk = hr.blocks_of(1, n, nb)
    for j in (0, 7, 19):
        fold = np.zeros((B, K), np.longdouble)
        for j2 in range(nb):
            if j2 != j:
                fold = fold + O[j2]
        direct = np.stack([R[(blk != j) & (batch == b)].astype(np.longdouble).sum(axis=0) for b in range(B)])
        assert np.abs(fold - direct).max() <= (n + 8) * hr.U * float(direct.max())


def test_symmetric_batches_are_left_alone():
    """every batch an exact copy of the same cells: at theta = 0 the batches' sums agree, W = 0 up to rounding, Z_corr = Z"""
    rng = np.random.default_rng(3)
    m, B, d, K = 120, 3, 6, 4
    Z1 = rng.normal(size=(m, d)) + 4.0 * np.eye(K, d)[rng.integers(0, K, m)]
    Z = np.tile(Z1, (B, 1))
    batch = np.repeat(np.arange(B), m)
    r = hr.harmony(Z, batch, n_clusters=K, theta=0.0, max_iter=3, epsilon_harmony=0.0)
    # Exactly, S_kb and N_kb are the same for every b, w0 = S / N and W = 0.  In fp64 a batch's S_kb and N_kb are sums of the same m terms
    # in another order, each within (m + 8) u sum |terms| <= (m + 8) u N max |Z| of the others', and w0 folds B of them (B + 8 more
    # roundings): |W_kb| <= (2 (m + 8) + B + 8) u max |Z| N / (N + lam).  The rows of R sum to 1, so Z_corr - Z = sum_k R_ik W_kb is within
    # the same, and every iteration corrects the original Z, so nothing accumulates over the three.
    bound = (2 * (m + 8) + B + 8) * hr.U * np.abs(Z).max()
    assert np.abs(r["Z_corr"] - Z).max() <= bound, (np.abs(r["Z_corr"] - Z).max(), bound)


def test_quality_on_the_planted_inputs(whole):
    for n in hr.WHOLE:
        Z, b, lab = whole[n]["data"]
        q = hr.QUALITY[n]
        before = hr.neighbour_shares(Z, b, lab)
        after = [hr.neighbour_shares(r["Z_corr"], b, lab) for r in whole[n]["seeds"]]
        sb, sl, cl = [a[0] for a in after], [a[1] for a in after], [a[2] for a in after]
        print(f"planted({n}): same batch {before[0]:.4f} -> {min(sb):.4f} .. {max(sb):.4f}; same label {before[1]:.4f} -> {min(sl):.5f} .. "
              f"{max(sl):.5f}, every cluster >= {min(cl):.4f}; iterations {[r['n_iter'] for r in whole[n]['seeds']]}")
        assert abs(before[0] - q["before"][0]) < 1e-4 and abs(before[1] - q["before"][1]) < 1e-4
        assert abs(max(sb) - q["same_batch_worst"]) < 1e-5 and abs(max(sb) - min(sb) - q["same_batch_spread"]) < 1e-5
        assert abs(min(sl) - q["same_label_worst"]) < 1e-5 and abs(max(sl) - min(sl) - q["same_label_spread"]) < 1e-5
        assert min(cl) >= q["min_cluster_label"]
        assert max(sb) < before[0] - 0.25 and max(sb) < 1.0 / 3 + 0.06 and min(sl) >= before[1]
        assert all(r["n_iter"] == 3 and r["converged"] for r in whole[n]["seeds"])
        d = hr.DECISIONS[n]
        r = whole[n]["seeds"][0]
        assert (r["n_iter"], tuple(r["rounds"]), r["converged"]) == (d["n_iter"], d["rounds"], d["converged"])


def test_rounding_spread_is_the_recorded_one(whole):
    for n in hr.WHOLE:
        a, w, ld = whole[n]["fixed"]
        rec = hr.SPREAD[n]
        for key, rel in (("Z_corr", True), ("Y", False), ("R", False)):
            got = max(hr.spread(a[key], ld[key], rel), hr.spread(w[key], ld[key], rel))
            print(f"planted({n}) {key}: spread {got:.2e}, recorded {rec[key]:.2e}")
            assert got <= rec[key] <= 1.25 * got
        a, w, ld = whole[n]["default"]
        assert len(a["all_objectives"]) == len(w["all_objectives"]) == len(ld["all_objectives"])
        got = max(hr.spread(a["all_objectives"], ld["all_objectives"]), hr.spread(w["all_objectives"], ld["all_objectives"]))
        print(f"planted({n}) objective: spread {got:.2e}, recorded {rec['objective']:.2e}")
        assert got <= rec["objective"] <= 1.25 * got


def test_stop_margins_and_start_gaps(whole):
    """the premises of the GPU's whole calls: no stop decision and no start assignment is within reach of rounding"""
    for n in hr.WHOLE:
        for r in whole[n]["default"]:
            assert (r["n_iter"], tuple(r["rounds"]), r["converged"]) == tuple(hr.DECISIONS[n][k] for k in ("n_iter", "rounds", "converged"))
            print(f"planted({n}): smallest stop margin {min(r['margins']):.2e}, smallest start gap {min(r['cos_gap']):.2e}")
            assert min(r["margins"]) >= 1e6 * hr.SPREAD[n]["objective"]
            # a dot of d = 10 terms on unit rows: (d + 1) u, for each of the two cosines
            assert min(r["cos_gap"]) > 1e6 * 2 * 11 * hr.U
        for r in whole[n]["fixed"]:
            assert min(r["cos_gap"]) > 1e6 * 2 * 11 * hr.U


def test_refusals_that_need_no_device():
    import sharp_amd as sa

    Z, b, _ = hr.planted(60)
    assert np.array_equal(sa.batch_of_blocks([np.zeros((5, 3)), np.zeros((5, 2))]), [0, 0, 0, 1, 1])
    bad = Z.copy()
    bad[7] = 0.0
    nan = Z.copy()
    nan[9, 2] = np.nan
    for args, kw, msg in (((bad, b), {}, r"a zero row in Z \(cell 7,"), ((nan, b), {}, r"a non-finite value in Z \(row 9,"),
                          ((Z, np.zeros(60, int)), {}, "one batch: nothing to integrate"), ((Z, b), {"n_clusters": 61}, "n_clusters exceeds the number of cells"),
                          ((Z, b), {"n_clusters": 1}, "need 2 <= n_clusters"), ((Z[:, :1], b), {}, "need 2 <= d <= 128 columns"),
                          ((np.ones((60, 129)), b), {}, "need 2 <= d <= 128 columns"), ((Z, b[:59]), {}, "batch must hold one label per cell"),
                          ((Z, b), {"sigma": 0.0}, "sigma must be > 0"), ((Z, b), {"theta": -1.0}, "theta must be >= 0"),
                          ((Z, b), {"lam": 0.0}, "lam must be > 0"), ((Z, b), {"n_blocks": 0}, "need 1 <= n_blocks <= 1024"),
                          ((Z, b), {"n_blocks": 1025}, "need 1 <= n_blocks <= 1024"), ((Z, b), {"max_iter": 0}, "need max_iter >= 1")):
        with pytest.raises(sa.SharpError, match="harmony_integrate: " + msg):
            sa.harmony_integrate(*args, **kw)
    from sharp_amd import harmony

    with pytest.raises(sa.SharpError, match=r"harmony_sums: an empty batch code \(1\)"):
        harmony._sums(np.ones((60, 2)), Z, np.where(b == 1, 0, b), 3)
    assert harmony._caps()[0] >= 64 and harmony._caps()[1] >= 129 * 2          # at least two clusters of the widest rows fit a tile


def test_the_library_refuses_again_without_the_package():
    from sharp_amd._lib import f64, i32, lib

    Z, b, _ = hr.planted(60)
    b = b.astype(np.int32)
    out = [np.zeros((60, 10)), np.zeros((256, 10)), np.zeros(10), np.zeros(10, np.int32)]
    ni, cv = C.c_int(), C.c_int()

    def call(Z=Z, b=b, n=60, d=10, B=3, K=2, sigma=0.1, theta=2.0, lam=1.0, max_iter=2, nb=20):
        rc = lib().sharp_harmony(f64(np.ascontiguousarray(Z)), n, d, i32(b), B, K, sigma, theta, lam, max_iter, 5, nb, 1e-5, 1e-4, 3, 1, f64(out[0]),
                                 f64(out[1]), f64(out[2]), i32(out[3]), C.byref(ni), C.byref(cv), None)
        return rc, lib().sharp_last_error()

    bad = Z.copy()
    bad[7] = 0.0
    nan = Z.copy()
    nan[9, 2] = np.inf
    for kw, msg in (({"Z": bad}, b"harmony_integrate: a zero row in Z (cell 7,"), ({"Z": nan}, b"a non-finite value in Z (cell 9,"),
                    ({"B": 1}, b"one batch: nothing to integrate"), ({"B": 4}, b"an empty batch code (3)"), ({"B": 2}, b"a batch code outside [0, batches)"),
                    ({"K": 61}, b"n_clusters exceeds the number of cells"), ({"K": 1}, b"need 2 <= n_clusters <= min(n, 256)"),
                    ({"d": 1}, b"need 2 <= d <= 128 columns"), ({"d": 129}, b"need 2 <= d <= 128 columns"), ({"B": 4097}, b"need 2 <= batches <= 4096"),
                    ({"sigma": -1.0}, b"sigma must be > 0"), ({"theta": float("nan")}, b"theta must be >= 0"), ({"lam": 0.0}, b"lam must be > 0"),
                    ({"nb": 0}, b"need 1 <= n_blocks <= 1024"), ({"max_iter": 0}, b"need max_iter >= 1")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
    slab, tile = C.c_int(), C.c_int()
    assert lib().sharp_harmony_caps(C.byref(slab), C.byref(tile)) == 0 and slab.value > 0 and tile.value > 0
    R = np.ones((60, 2))
    assert lib().sharp_harmony_correct(f64(Z), f64(R), i32(b), f64(np.zeros((1, 2, 10))), 60, 10, 2, 1, f64(out[0])) != 0
    assert b"harmony_correct: one batch: nothing to integrate" in lib().sharp_last_error()
    assert lib().sharp_harmony_assign(f64(Z), f64(Z[:2]), i32(b), None, 60, 10, 2, 3, 5, 4, 0.1, 0, f64(R), None) != 0
    assert b"harmony_assign: need 0 <= i0 <= i1 <= n" in lib().sharp_last_error()
