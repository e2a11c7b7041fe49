"""The Leiden specification of DESIGN.md §25 in numpy, on the functions of _louvain_ref.py (§18's rules 1 - 4 are used unchanged): a
level's move phase from a given start (L1), the refinement of the level's partition P into well-connected sub-communities (L2), the
aggregation by sub-community with the parent partition as the next start (L3) and the split of the returned partition into connected
components (L4).  This is the project's own deterministic form; no parity with leidenalg, igraph or scanpy is claimed.  Every sum of
weights is an int64 sum, every fp64 expression is written in the operation order the kernels use, so the GPU tests ask for equal bits.
The reference asserts the invariants of L2 as it runs."""
import numpy as np

import _louvain_ref as lv
from _louvain_ref import MAX_FAILS, MAX_LEVELS, MAX_ROUNDS, TOL, _group_sum, _rows, _scatter_sum

MAX_REFINE_ROUNDS = 200
REFINE_ROUND0 = 1 << 30                                        # h' = h at the round number 2^30 + r: the move phase never gets there


# ---- L1: a level's move phase from comm0 ----------------------------------------------------------------------------------------------
def level(rp, col, q, gamma, seed, lev, comm0=None, tol=TOL, max_rounds=MAX_ROUNDS, max_fails=MAX_FAILS):
    """§18's level started from comm0 (None: the singletons): (comm, rounds, Q of the accepted state)"""
    n = len(rp) - 1
    k = lv.strengths(rp, q)
    comm = np.arange(n, dtype=np.int32) if comm0 is None else np.asarray(comm0, np.int32).copy()
    tot, _, _, Q = lv.state(rp, col, q, comm, gamma, k)
    rounds = fails = 0
    while rounds < max_rounds and fails < max_fails:
        prop = lv.move(rp, col, q, comm, gamma, seed, lev, rounds, k, tot)
        rounds += 1
        tot2, _, _, Q2 = lv.state(rp, col, q, prop, gamma, k)
        if Q2 > Q + tol:
            comm, tot, Q, fails = prop, tot2, Q2, 0
        else:
            fails += 1
    return comm, rounds, Q


# ---- L2: the refinement ---------------------------------------------------------------------------------------------------------------
def subtotals(rp, col, q, P, ref, k=None):
    """(stot, size, ext, e, totP): per sub-community id the strength, the members and the weight towards the rest of its community;
    per vertex the weight towards its community; per community id the strength"""
    rp, col, q = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(q, np.int64)
    P, ref = np.asarray(P, np.int64), np.asarray(ref, np.int64)
    n = rp.size - 1
    row = _rows(rp)
    k = lv.strengths(rp, q) if k is None else np.asarray(k, np.int64)
    same = (P[row] == P[col]) & (row != col)
    out = same & (ref[col] != ref[row])
    return (_scatter_sum(ref, k, n), np.bincount(ref, minlength=n).astype(np.int64), _scatter_sum(ref[row[out]], q[out], n),
            _scatter_sum(row[same], q[same], n), _scatter_sum(P, k, n))


def flags(P, ref, k, sub, gamma):
    """(eligible per vertex, well connected per sub-community id); an id without members is not well connected"""
    stot, size, ext, e, totP = sub
    P, ref, k = np.asarray(P, np.int64), np.asarray(ref, np.int64), np.asarray(k, np.int64)
    m2 = float(int(k.sum()))
    kf = k.astype(np.float64)
    elig = (size[ref] == 1) & (e.astype(np.float64) >= ((gamma * kf) * (totP[P] - k).astype(np.float64)) / m2)
    # (a sub-community with members holds the vertex of its id: P of that vertex is its community)
    well = (size > 0) & (ext.astype(np.float64) >= ((gamma * stot.astype(np.float64)) * (totP[P] - stot).astype(np.float64)) / m2)
    return elig, well


def refine_round(rp, col, q, P, ref, gamma, seed, lev, r, k=None, detail=None):
    """one round from the state ref: (proposal, moved, wanting); wanting = the vertices that hold a candidate with gain > 0, whatever
    the bits say.  detail: a dict that receives the round's flags and candidates"""
    rp, col, q = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(q, np.int64)
    P, ref = np.asarray(P, np.int64), np.asarray(ref, np.int64)
    n = rp.size - 1
    row = _rows(rp)
    k = lv.strengths(rp, q) if k is None else np.asarray(k, np.int64)
    m2 = float(int(k.sum()))
    sub = subtotals(rp, col, q, P, ref, k)
    stot = sub[0]
    elig, well = flags(P, ref, k, sub, gamma)
    same = (P[row] == P[col]) & (row != col)
    key, kin = _group_sum(row[same] * n + ref[col[same]], q[same])
    pv, ps = key // n, key % n
    cand = elig[pv] & (ps != ref[pv]) & well[ps]
    gain = kin.astype(np.float64) - ((gamma * k[pv].astype(np.float64)) * stot[ps].astype(np.float64)) / m2
    pos = cand & (gain > 0.0)
    wanting = int(np.unique(pv[pos]).size)
    rnd = REFINE_ROUND0 + int(r)
    ok = pos & (lv.hbit(seed, lev, rnd, ref[pv]) == 1) & (lv.hbit(seed, lev, rnd, ps) == 0)
    if detail is not None:
        detail.update(eligible=elig, well=well, vertex=pv, target=ps, candidate=cand, excluded=elig[pv] & (ps != ref[pv]) & ~well[ps])
    pv, ps, gain = pv[ok], ps[ok], gain[ok]
    o = np.lexsort((ps, -gain, pv))
    pv, ps = pv[o], ps[o]
    first = np.flatnonzero(np.r_[True, pv[1:] != pv[:-1]]) if pv.size else np.zeros(0, np.int64)
    bv, bs = pv[first], ps[first]
    prop = ref.copy()
    prop[bv] = bs
    # the invariant of the bits: a sub-community that gains loses nothing
    assert not np.isin(ref[bv], bs).any()
    return prop.astype(np.int32), int(bv.size), wanting


def check_refinement(rp, col, P, ref):
    """every sub-community lies inside one community of P and is connected in the graph"""
    P, ref = np.asarray(P, np.int64), np.asarray(ref, np.int64)
    n = len(rp) - 1
    assert np.unique(ref * n + P).size == np.unique(ref).size, "a sub-community across two communities"
    assert np.unique(split(rp, col, ref)).size == np.unique(ref).size, "a sub-community that is not connected"


def refine(rp, col, q, P, gamma, seed, lev, max_refine_rounds=MAX_REFINE_ROUNDS, check=True, trace=None):
    """(ref, counted rounds): rounds from the singletons until no vertex holds a candidate with gain > 0 (that round is not counted)
    or the cap.  trace: a list that receives (state, proposal) of every counted round"""
    n = len(rp) - 1
    k = lv.strengths(rp, q)
    ref = np.arange(n, dtype=np.int32)
    rounds = 0
    while rounds < max_refine_rounds:
        prop, moved, wanting = refine_round(rp, col, q, P, ref, gamma, seed, lev, rounds, k)
        if wanting == 0:
            break
        if trace is not None:
            trace.append((ref, prop))
        ref = prop
        rounds += 1
    if check:
        check_refinement(rp, col, P, ref)
    return ref, rounds


# ---- L3 / L4: components within a labelling -------------------------------------------------------------------------------------------
def split(rp, col, label):
    """out[v] = the smallest vertex of v's component in the graph restricted to the entries whose two ends carry the same label
    (self-loops ignored)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    rp, col, label = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(label, np.int64)
    n = rp.size - 1
    row = _rows(rp)
    keep = (label[row] == label[col]) & (row != col)
    A = csr_matrix((np.ones(int(keep.sum()), np.int8), (row[keep], col[keep])), shape=(n, n))
    comp = connected_components(A, directed=False)[1]
    low = np.full(n, n, np.int64)
    np.minimum.at(low, comp, np.arange(n))
    return low[comp].astype(np.int32)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def leiden_q(rp, col, q, gamma=1.0, seed=10, tol=TOL, max_levels=MAX_LEVELS, max_rounds=MAX_ROUNDS, max_fails=MAX_FAILS,
             max_refine_rounds=MAX_REFINE_ROUNDS, check=True, trace=None):
    """the driver on an integer-weighted CSR: {"membership" (1 .. G), "n_communities", "modularity", "levels": [{"n", "communities",
    "sub_communities", "rounds", "refine_rounds", "modularity", "membership" (the 0-based rank of the community P of the input's
    vertices)}]}.  trace: a list that receives per level {"graph": (rp, col, q), "comm0", "P", "ref", "rounds": [(state, proposal)]}"""
    rp0, col0, q0 = rp, col, q
    n0 = len(rp) - 1
    vmap = np.arange(n0, dtype=np.int64)
    comm0 = None
    levels = []
    for lev in range(max_levels):
        n = len(rp) - 1
        if check and comm0 is not None:
            assert np.array_equal(split(rp, col, comm0), comm0), "a level that starts from a disconnected community"
        P, rounds, Q = level(rp, col, q, gamma, seed, lev, comm0, tol, max_rounds, max_fails)
        rtrace = [] if trace is not None else None
        ref, rr = refine(rp, col, q, P, gamma, seed, lev, max_refine_rounds, check, rtrace)
        if trace is not None:
            trace.append({"graph": (rp, col, q), "comm0": comm0, "P": P, "ref": ref, "rounds": rtrace})
        ids, rank = np.unique(P, return_inverse=True)
        sub = int(np.unique(ref).size)
        levels.append({"n": n, "communities": int(ids.size), "sub_communities": sub, "rounds": rounds, "refine_rounds": rr, "modularity": Q,
                       "membership": rank.reshape(-1)[vmap].astype(np.int32)})
        if sub == n or lev + 1 == max_levels:
            break
        crp, ccol, cq, new = lv.aggregate(rp, col, q, ref)
        parent = np.zeros(sub, np.int64)
        parent[new[np.asarray(ref, np.int64)]] = P
        vmap = new[np.asarray(ref, np.int64)[vmap]]
        comm0 = split(crp, ccol, parent)
        rp, col, q = crp, ccol, cq
    final = split(rp, col, P)[vmap]
    mem = lv.relabel_by_size(final)
    return {"membership": mem, "n_communities": int(mem.max()), "modularity": lv.modularity_q(rp0, col0, q0, mem, gamma), "levels": levels,
            "seed": seed}


def leiden(rp, col, val, gamma=1.0, seed=10, **kw):
    """the driver on a float-weighted symmetric CSR without diagonal entries"""
    q = lv.quantise(rp, col, val)[0]
    return leiden_q(*lv.drop_zeros(rp, col, q), gamma, seed, **kw)


def int_graph(rp, col, val):
    return lv.drop_zeros(rp, col, lv.quantise(rp, col, val)[0])


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def cliques_across_a_gap(size=6):
    """two cliques labelled as one community that touch only through a vertex of another community: (rp, col, q, P).  Vertices
    0 .. size - 1 and size .. 2 size - 1 are the cliques (P = 0); 2 size joins the last of the first to the first of the second and
    hangs on 2 size + 1 (P = 2 size for both)"""
    a, b = np.triu_indices(size, 1)
    g = 2 * size
    i = np.r_[a, a + size, size - 1, g, g]
    j = np.r_[b, b + size, g, size, g + 1]
    rp, col, q = lv.csr_from_pairs(g + 2, i, j, np.full(i.size, 1 << 20, np.int64))
    return rp, col, q, np.r_[np.zeros(g, np.int32), np.full(2, g, np.int32)]


def table(seeds=(10, 11, 12)):
    """the rows of DESIGN.md §25's table: per case and seed the Louvain reference's and this reference's Q and communities, and the levels"""
    blobs, gauss, planted = lv.blobs_graph()[:3], lv.gaussian_graph()[:3], lv.planted()[:3]
    cases = [("gaussian 2000 x 50, K = 14", gauss, (1.0, 2.0, 4.0)), ("blobs 1500 x 10", blobs, (1.0, 4.0)), ("path 1025", lv.path(), (1.0,)),
             ("planted 8 x 64", planted, (1.0, 3.0)), ("ring of 30 six-cliques", lv.ring_of_cliques(), (1.0,)), ("star of 3000", lv.star(), (1.0,))]
    rows = []
    for name, g, gammas in cases:
        for gamma in gammas:
            a = [lv.louvain(*g, gamma, s) for s in seeds]
            b = [leiden(*g, gamma, s) for s in seeds]
            rows.append((name, gamma, " / ".join(f"{r['modularity']:.6f} ({r['n_communities']})" for r in a),
                         " / ".join(f"{r['modularity']:.6f} ({r['n_communities']})" for r in b),
                         " / ".join(str(len(r["levels"])) for r in b),
                         "%d-%d" % (min(l["refine_rounds"] for r in b for l in r["levels"]), max(l["refine_rounds"] for r in b for l in r["levels"])),
                         sum(x["modularity"] < y["modularity"] for x, y in zip(b, a))))
    return rows


if __name__ == "__main__":
    for row in table():
        print("| " + " | ".join(str(x) for x in row) + " |")
