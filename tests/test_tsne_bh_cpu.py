"""The Barnes-Hut specification of DESIGN.md §10 (tests/_tsne_bh_ref.py) against bhtsne's SPTree restated literally, and the exact
gradient of tests/_tsne_ref.py; no GPU needed."""
import numpy as np
import pytest
import scipy.sparse as sp

import _tsne_bh_ref as bh
import _tsne_ref as ref


def _mixture(n, dims, seed, groups=8):
    """the generator of DESIGN.md's measurement: 8 Gaussian clusters, centres N(0, 25^2), spread 3"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 25, size=(groups, dims))
    return centres[rng.integers(0, groups, n)] + 3 * rng.normal(size=(n, dims))


def _p(n, seed):
    P = sp.random(n, n, density=8.0 / n, random_state=seed, format="csr")
    P = (P + P.T).tocsr()
    P.sort_indices()
    return P / P.sum()


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_compressed_tree_equals_sptree(dims):
    Y = _mixture(1500, dims, 40 + dims)
    P = _p(1500, dims)
    for theta in (0.25, 0.5, 0.8):
        g, Z = bh.bh_gradient(P, Y, theta, return_z=True)
        gs, Zs = bh.sptree_gradient(P, Y, theta, return_z=True)
        assert abs(Z - Zs) <= 1e-12 * Zs, (theta, Z, Zs)
        assert np.abs(g - gs).max() <= 1e-12 * np.abs(gs).max(), theta


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_theta_zero_is_exact(dims):
    Y = _mixture(700, dims, 50 + dims)
    P = _p(700, 7 + dims)
    ge, Ze = ref.gradient(P, Y, return_z=True)
    for f in (bh.bh_gradient, bh.sptree_gradient):
        g, Z = f(P, Y, 0.0, return_z=True)
        assert abs(Z - Ze) <= 1e-12 * Ze
        assert np.abs(g - ge).max() <= 1e-10 * np.abs(ge).max()


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_accepted_nodes_partition_the_points(dims):
    """Per point, the nodes taken as summaries and its own skipped leaf tile the sorted rows [0, n) without overlap.  A summary
    may hold the point itself (its cell is accepted from inside); below theta = 1 / (2 sqrt(dims)) that cannot happen, so at
    theta = 0.25 the summaries of duplicate-free data hold exactly the other n - 1 points."""
    Y = _mixture(1200, dims, 60 + dims)
    Y[100] = Y[7]                                   # exact duplicates: one leaf of three points
    Y[900] = Y[7]
    n = Y.shape[0]
    for theta in (0.25, 0.5, 0.8):
        _, _, _, trail, tree = bh.bh_repulsion(Y, theta, record=True)
        start, end, cnt, low = tree[7], tree[8], tree[1], tree[4]
        pt, node = trail[:, 0], trail[:, 1]
        o = np.lexsort((start[node], pt))
        pt, node = pt[o], node[o]
        first = np.r_[True, pt[1:] != pt[:-1]]
        last = np.r_[pt[1:] != pt[:-1], True]
        assert np.array_equal(np.unique(pt), np.arange(n))
        assert (start[node[first]] == 0).all() and (end[node[last]] == n).all()
        assert (end[node[:-1]][~last[:-1]] == start[node[1:]][~last[:-1]]).all()
        held = np.bincount(pt, weights=cnt[node] * (trail[o, 2] == 0), minlength=n)
        if theta == 0.25:
            own = np.array([cnt[(low == i)].sum() for i in range(n)])   # the leaf skipped for its lowest index
            assert np.array_equal(held, n - own)
            assert own[7] == 3 and own[100] == 0 and (np.delete(own, [7, 100, 900]) == 1).all()


def test_duplicates_share_a_leaf_and_count_in_it():
    Y = _mixture(300, 2, 70)
    Y[[10, 20, 30]] = Y[5]
    com, cnt, hw, leaf, low, skip, perm, start, end = bh.bh_tree(Y)
    k = np.flatnonzero(leaf & (low == 5))
    assert k.size == 1 and cnt[k[0]] == 4 and np.array_equal(np.sort(perm[start[k[0]]:end[k[0]]]), [5, 10, 20, 30])
    assert leaf.sum() == 297 and len(skip) <= 2 * 300 and skip[0] == len(skip)
    # the point with the lowest index skips its leaf; its twins take it as a summary of 4 at distance 0
    rep, z, _ = bh.bh_repulsion(Y, 0.0)
    ex = 1.0 / (1.0 + ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(ex, 0.0)
    assert np.isclose(z[5], ex[5].sum() - 3, rtol=1e-12)
    assert np.isclose(z[10], ex[10].sum() + 1, rtol=1e-12)


def test_errors_rise_with_theta_on_the_cluster_mixture():
    """the numbers DESIGN.md §10 quotes for a 2 000-point 8-cluster 2-D mixture (Z within 5 %, rep / Z within 10 % at theta = 0.5)"""
    Y = _mixture(2000, 2, 3)
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    Q = 1.0 / (1.0 + D)
    np.fill_diagonal(Q, 0.0)
    Ze = Q.sum()
    Q2 = Q * Q
    re = (Q2.sum(1)[:, None] * Y - Q2 @ Y) / Ze
    ez, er, vis = [], [], []
    for theta in (0.2, 0.5, 0.8):
        rep, z, v = bh.bh_repulsion(Y, theta)
        ez.append(abs(z.sum() - Ze) / Ze)
        er.append(np.linalg.norm(rep / z.sum() - re) / np.linalg.norm(re))
        vis.append(v.mean())
    assert ez[0] < ez[1] < ez[2] and er[0] < er[1] < er[2] and vis[0] > vis[1] > vis[2]
    assert ez[1] <= 0.05 and er[1] <= 0.1


def test_unknown_repulsion_is_refused_before_any_device_call():
    import sharp_amd

    with pytest.raises(sharp_amd.SharpError, match="repulsion"):
        sharp_amd.Rtsne(np.zeros((10, 3)), repulsion="fft")
