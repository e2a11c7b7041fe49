"""numpy fp64 reference of the Barnes-Hut repulsion in DESIGN.md §10 (test infrastructure only: the product never imports it).

sptree_gradient: bhtsne's SPTree restated literally (points inserted in index order, node capacity 1, half-widths, an exact
duplicate absorbed into the leaf that holds its twin, a leaf subdivided when a second distinct point arrives), then its
computeNonEdgeForces.  bh_gradient: the specification the GPU follows (quantised Morton keys, a compressed tree, finest-cell leaves),
built here by plain recursion over the sorted keys.  Both trees are walked in preorder with a skip index per node, all points at once."""
import numpy as np

import _tsne_ref as ref

BITS = {1: 63, 2: 32, 3: 21}   # levels below the root: 64-bit keys


def attraction(P, Y):
    n, dims = Y.shape
    P = P.tocoo()
    diff = Y[P.row] - Y[P.col]
    q = P.data / (1.0 + (diff ** 2).sum(1))
    attr = np.zeros_like(Y)
    for k in range(dims):
        attr[:, k] = np.bincount(P.row, weights=q * diff[:, k], minlength=n)
    return attr


def _walk(Y, com, cnt, hw, leaf, low, skip, theta, record=False):
    """computeNonEdgeForces for every point over a preorder layout: a leaf whose `low` is the point itself is skipped; a leaf, or a
    node with hw / sqrt(D) < theta, is a summary (cnt q to z, cnt q^2 (y_i - com) to rep), the walk then jumps to skip; otherwise it
    enters the first child.  Returns rep, zrow, visits per point and (record) the (point, node, skipped) triples."""
    n, dims = Y.shape
    M = skip[0]
    k = np.zeros(n, np.int64)
    rep = np.zeros((n, dims))
    z = np.zeros(n)
    visits = np.zeros(n, np.int64)
    trail = []
    pts = np.arange(n)
    while True:
        a = pts[k < M]
        if a.size == 0:
            break
        kk = k[a]
        visits[a] += 1
        own = leaf[kk] & (low[kk] == a)
        d = Y[a] - com[kk]
        D = np.zeros(a.size)
        for c in range(dims):
            D = D + d[:, c] * d[:, c]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = ~own & (leaf[kk] | (hw[kk] / np.sqrt(D) < theta))
        q = 1.0 / (1.0 + D[acc])
        mult = cnt[kk[acc]] * q
        z[a[acc]] += mult
        mult = mult * q
        rep[a[acc]] += mult[:, None] * d[acc]
        if record:
            trail.append(np.stack([a[acc | own], kk[acc | own], own[acc | own].astype(np.int64)], 1))
        k[a] = np.where(acc | own, skip[kk], kk + 1)
    return rep, z, visits, (np.concatenate(trail) if trail else np.zeros((0, 3), np.int64))


# ---- bhtsne's SPTree, literally -------------------------------------------------------------------------------------------------------
class _SPTree:
    def __init__(self, data, corner, width):
        self.data, self.corner, self.width = data, corner, width
        self.D = len(corner)
        self.is_leaf, self.size, self.cum_size = True, 0, 0
        self.index = []
        self.com = [0.0] * self.D
        self.children = []

    def contains(self, p):
        for d in range(self.D):
            if self.corner[d] - self.width[d] > p[d] or self.corner[d] + self.width[d] < p[d]:
                return False
        return True

    def insert(self, i):
        p = self.data[i]
        if not self.contains(p):
            return False
        self.cum_size += 1
        m1 = (self.cum_size - 1) / self.cum_size
        m2 = 1.0 / self.cum_size
        self.com = [self.com[d] * m1 + m2 * p[d] for d in range(self.D)]
        if self.is_leaf and self.size < 1:
            self.index.append(i)
            self.size += 1
            return True
        if any(self.data[j] == p for j in self.index[: self.size]):   # a duplicate is counted here and stored nowhere
            return True
        if self.is_leaf:
            self.subdivide()
        for c in self.children:
            if c.insert(i):
                return True
        return False

    def subdivide(self):
        for i in range(2 ** self.D):
            corner, div = [], 1
            for d in range(self.D):
                corner.append(self.corner[d] - .5 * self.width[d] if (i // div) % 2 == 1 else self.corner[d] + .5 * self.width[d])
                div *= 2
            self.children.append(_SPTree(self.data, corner, [.5 * w for w in self.width]))
        for j in self.index[: self.size]:
            ok = False
            for c in self.children:
                if not ok:
                    ok = c.insert(j)
        self.index, self.size, self.is_leaf = [], 0, False


def sptree(Y):
    """bhtsne's SPTree of Y, flattened in preorder (non-empty nodes only: computeNonEdgeForces returns at cum_size == 0)"""
    n, D = Y.shape
    data = [tuple(float(v) for v in row) for row in Y]
    mean = [sum(Y[i, d] for i in range(n)) / n for d in range(D)]
    width = [max(Y[:, d].max() - mean[d], mean[d] - Y[:, d].min()) + 1e-5 for d in range(D)]
    root = _SPTree(data, mean, width)
    for i in range(n):
        root.insert(i)
    com, cnt, hw, leaf, low, skip = [], [], [], [], [], []

    def flat(t):
        k = len(com)
        com.append(t.com)
        cnt.append(t.cum_size)
        mw = 0.0
        for w in t.width:
            mw = mw if mw > w else w
        hw.append(mw)
        leaf.append(t.is_leaf)
        low.append(t.index[0] if t.is_leaf and t.size == 1 else -1)
        skip.append(0)
        for c in t.children:
            if c.cum_size > 0:
                flat(c)
        skip[k] = len(com)

    flat(root)
    return (np.array(com), np.array(cnt, np.float64), np.array(hw), np.array(leaf), np.array(low, np.int64), np.array(skip, np.int64))


def sptree_gradient(P, Y, theta, return_z=False):
    rep, z, _, _ = _walk(Y, *sptree(Y), theta)
    Z = z.sum()
    g = attraction(P, Y) - rep / Z
    return (g, Z) if return_z else g


# ---- the specification the GPU follows --------------------------------------------------------------------------------------------------
def keys(Y):
    """the finest cell of every row as a Morton key: upper halves first, dimension k at bit k of every digit (bhtsne's child order)"""
    n, dims = Y.shape
    bits = BITS[dims]
    mean = Y.sum(0) / n
    w = np.maximum(Y.max(0) - mean, mean - Y.min(0)) + 1e-5
    lo = mean - w
    scale = 2.0 ** bits / (2.0 * w)
    lim = 2.0 ** bits
    top = np.uint64((1 << bits) - 1)
    K = np.zeros(n, np.uint64)
    for k in range(dims):
        t = (Y[:, k] - lo[k]) * scale[k]
        u = np.where((t >= 0) & (t < lim), t, 0.0).astype(np.uint64)
        u[t >= lim] = top
        c = top - u
        for b in range(bits):
            K |= ((c >> np.uint64(b)) & np.uint64(1)) << np.uint64(b * dims + k)
    return K, w.max()


def _lcp(a, b, dims):
    bits = BITS[dims]
    if a == b:
        return bits
    return bits - 1 - (int(a ^ b).bit_length() - 1) // dims


def bh_tree(Y):
    """the compressed tree in preorder: a cell whose points all fall in one child is not a node of its own (the chain is one node at
    the level of its deepest cell); a run of equal keys is one leaf, its `low` the lowest index in it.  Returns
    (com, cnt, hw, leaf, low, skip, perm, start, end): start / end are the node's rows in the key order perm."""
    n, dims = Y.shape
    bits = BITS[dims]
    K, wmax = keys(Y)
    perm = np.argsort(K, kind="stable")
    Ks = [int(v) for v in K[perm]]
    Ys = Y[perm]
    nodes = []   # [start, end, level, is_leaf, skip]

    def rec(s, e):
        g = _lcp(Ks[s], Ks[e - 1], dims)
        k = len(nodes)
        nodes.append([s, e, g, g >= bits, 0])
        if g < bits:
            shift = (bits - g - 1) * dims
            c = s
            while c < e:
                dig = (Ks[c] >> shift) & ((1 << dims) - 1)
                c2 = c
                while c2 < e and (Ks[c2] >> shift) & ((1 << dims) - 1) == dig:
                    c2 += 1
                rec(c, c2)
                c = c2
        nodes[k][4] = len(nodes)

    rec(0, n)
    start = np.array([v[0] for v in nodes])
    end = np.array([v[1] for v in nodes])
    level = np.array([v[2] for v in nodes])
    leaf = np.array([v[3] for v in nodes])
    skip = np.array([v[4] for v in nodes], np.int64)
    cnt = (end - start).astype(np.float64)
    com = np.array([Ys[s:e].sum(0) for s, e in zip(start, end)]) / cnt[:, None]
    low = np.where(leaf, perm[start], -1)
    hw = wmax * 2.0 ** (-level.astype(np.float64))
    return com, cnt, hw, leaf, low, skip, perm, start, end


def bh_repulsion(Y, theta, record=False):
    """rep (n x dims), zrow (n), visits (n) and, with record, the (point, node, skipped) triples and the tree"""
    tree = bh_tree(Y)
    rep, z, visits, trail = _walk(Y, *tree[:6], theta, record=record)
    return (rep, z, visits, trail, tree) if record else (rep, z, visits)


def bh_gradient(P, Y, theta, return_z=False):
    """dY_i = attr_i - rep_i / Z, Z = sum_i z_i, the repulsion from the compressed tree at theta"""
    rep, z, _ = bh_repulsion(Y, theta)
    Z = z.sum()
    g = attraction(P, Y) - rep / Z
    return (g, Z) if return_z else g


def optimise(P, Y0, theta, **kw):
    """_tsne_ref.optimise with the Barnes-Hut gradient (and its Z in the KL)"""
    saved = ref.gradient, ref.kl
    state = {}

    def grad(Pm, Y):
        g, Z = bh_gradient(Pm, Y, theta, return_z=True)
        state["Z"] = Z
        return g

    def kl(Pm, Y, per_point=False):
        _, Z = bh_gradient(Pm, Y, theta, return_z=True)
        r, c, p = ref._pairs(Pm)
        Q = 1.0 / (1.0 + ((Y[r] - Y[c]) ** 2).sum(1)) / Z
        terms = p * np.log((p + ref.FLT_MIN) / (Q + ref.FLT_MIN))
        return np.bincount(r, weights=terms, minlength=Y.shape[0]) if per_point else terms.sum()

    ref.gradient, ref.kl = grad, kl
    try:
        return ref.optimise(P, Y0, **kw)
    finally:
        ref.gradient, ref.kl = saved
