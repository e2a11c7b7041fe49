"""rank_genes_groups on the GPU (csrc/rank_genes.hip) against tests/_rank_genes_ref.py.

The integers (2R, the tie terms, the non-zero counts) are compared bit for bit.  Every float is compared within a bound derived here
from the double operations between those integers (or the sums) and the output; eps = 2^-53, "lg" = 1 under log1p.
  value   a transformed value may differ from numpy's by the two log1p implementations: 4 ulp = 8 eps relative are allowed under log1p,
          nothing otherwise (one product of the same doubles).  rank_margin() (CPU) states that no rank depends on those bits.
  sums    k stored terms added in any order: (k - 1) eps sum|x|; with the value term, e_S = (k + 8 lg) eps sum|x|.
  means   e_S / n_g + 2 eps |mean| (the division, the reference's own rounding).  means_ref against the rest is (T - S_g) / n_r with T
          the groups' sums added in group order: ((k_all + G + 2 + 8 lg) eps sum_all|x|) / n_r + 2 eps |mean|.
  pct, auc  integers below 2^53 and one division: 2 eps relative.
  z       T = (N^3 - N - ties) / (N^3 - N): two exact conversions (below 2^53 at these sizes) and a division, eps; sigma^2 = n_g n_r (N +
          1) / 12 T: four more; the square root halves that and adds one; the numerator is an exact half-integer; the division adds
          one: under 5 eps, and the reference's rounding from longdouble: 8 eps |z| is allowed.
  p       erfc at x = |z| / sqrt 2 has relative condition kappa = 2 x / (sqrt(pi) erfcx(x)); x carries z's 8 eps and 2 eps from the
          product with the rounded constant; both erfc implementations are allowed 8 eps: p (10 kappa + 16) eps, plus 2^-1000 where p
          leaves the normal range.
  lfc     a = expm1(mean) + 1e-9 (mean + 1e-9 without log1p): da = e^mean dmean + 9 eps |a| (expm1 within 4 ulp, the sum); the
          quotient adds eps, log2 divides by ln 2 and is allowed 4 ulp: (da / |a| + db / |b| + eps) / ln 2 + 9 eps |lfc|.
  t       e_Q = (k + 2 + 16 lg) eps sum x^2 for the sum of squares; ss = Q - n mean^2: dss = e_Q + n (2 |mean| dmean + 3 eps mean^2) +
          eps Q; v = ss / (n - 1) / n: dv = dss / ((n - 1) n) + 3 eps v; dt = (dmean_g + dmean_r + eps |md|) / sqrt(a + b) + |t| ((da +
          db) / (2 (a + b)) + 4 eps); ddf / df = (2 (a + b)(da + db)) / (a + b)^2 + (2 a da / (n_g - 1) + 2 b db / (n_r - 1)) / den + 8
          eps.  The p-value is compared at the corners (|t| -+ dt, df -+ ddf) of the reference's own function, plus the relative
          error of the continued fraction's prefactor, 8 eps (|lgamma(a + b)| + |lgamma(a)| + |lgamma(b)| + |a ln x| + |b ln(1 - x)| +
          8): relative to p where the fraction gives p itself (x < (a + 1) / (a + b + 2)), to 1 - p where it gives the complement;
          and 32 eps for the reference.
  adj     Benjamini-Hochberg is checked as a function: the reference's bh() of the GPU's own p-values, 4 eps relative (one product,
          one quotient); the p-values themselves are checked above.
  order   exact, on cases whose neighbouring reference scores are tied exactly or further apart than the sum of their bounds
          (score_margin asserts it on the CPU for every case and gene).
  marker  get_marker_genes computes its AUROC from a mean rank: mr = (s2 / 2 + zero_rank2 zc / 2) / n1, R1 = mr n1, auc = (R1 - n1 (n1 +
          1) / 2) / (n1 n2): six roundings on numbers up to R1 <= n1 (n1 + 1) / 2 + n1 n2, so 8 eps (1 + (n1 + 1) / (2 n2)), plus 2
          eps for auc here.
The largest ratio of a difference to its bound is printed per quantity.  Observed on one MI355X, over all cases: means 0.12,
means_ref 0.11, pct 0, auc 0, logfoldchanges 0.11, z 0.32, Wilcoxon p 0.54, t 0.11, t-test p 0.24, pvals_adj 0, the marker AUROC 0; the
reference's smallest score gap is 3.5e7 times the bounds."""
import math

import numpy as np
import pytest
from scipy.special import erfcx, gammaln
from scipy.stats import t as tdist

import _expr_pca_ref as E
import _rank_genes_ref as R

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def chunk(sa):
    from sharp_amd import expr_pca

    return expr_pca._row_caps()[0]


@pytest.fixture(scope="module")
def cases(chunk):
    """name -> (X, codes, G, transform options); the references are computed once per (case, method, ref) and shared"""
    on, off = {"normalize_total": 1e4, "log1p": True}, {"normalize_total": None, "log1p": False}
    c = {}
    X, codes = R.count_case(2 * chunk + 1, 200, 7, 21, chunk)
    c["counts1025"] = (X, codes, 7, on)
    X, codes = R.raw_case(3001, 300, 7, 22, chunk, sizes=[1, 500, 500, 500, 500, 500, 500])
    c["raw3001"] = (X, codes, 7, off)
    X, codes = R.raw_case(2 * chunk + 1, 40, 2, 23, chunk)
    c["two1025"] = (X, codes, 2, off)
    X, codes = R.pairs_case(chunk)
    c["pairs2048"] = (X, codes, 1024, off)
    assert R.rank_margin(c["counts1025"][0]) > 2.0 ** -40
    return c


_memo = {}


def _ref(cases, name, method="wilcoxon", ref=-1, **kw):
    key = (name, method, ref, tuple(sorted(kw.items())))
    if key not in _memo:
        X, codes, G, opt = cases[name]
        _memo[key] = R.reference(X, codes, G, method=method, ref=ref, **opt, **kw)
    return _memo[key]


def _call(sa, cases, name, method="wilcoxon", ref=-1, blocks=None, **kw):
    X, codes, G, opt = cases[name]
    return sa.rank_genes_groups(X if blocks is None else blocks, codes, method=method, reference="rest" if ref < 0 else ref, **opt, **kw)


def _ratio(what, got, want, bound, live=None):
    """asserts |got - want| <= bound where live; returns and prints the largest ratio"""
    live = np.isfinite(want) if live is None else live
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    d = np.abs(got[live] - want[live])
    b = bound[live] if isinstance(bound, np.ndarray) else np.full(d.shape, bound)
    ratio = float((d / np.maximum(b, 1e-320)).max()) if d.size else 0.0
    print(f"  {what}: largest |gpu - reference| {d.max() if d.size else 0.0:.3e}, largest ratio to its bound {ratio:.3f}")
    assert (d <= b).all(), what
    return ratio


def _bounds(r, lg, rest, G):
    """the bounds of the docstring as G x m arrays, from the reference's premises"""
    ng, nr = r["n_g"][:, None].astype(float), np.maximum(r["n_r"][:, None].astype(float), 1.0)
    val = 8.0 * lg
    eS = (r["stored"] + val) * EPS * r["sumabs"]
    dmg = eS / ng + 2 * EPS * np.abs(r["means"])
    if rest:
        k_all, s_all = r["stored"] + r["stored_ref"], r["sumabs"] + r["sumabs_ref"]
        dmr = (k_all + G + 2 + val) * EPS * s_all / nr + 2 * EPS * np.abs(r["means_ref"])
        eQr = (k_all + G + 4 + 2 * val) * EPS * (r["sumsq"] + r["sumsq_ref"])
    else:
        dmr = (r["stored_ref"] + val) * EPS * r["sumabs_ref"] / nr + 2 * EPS * np.abs(r["means_ref"])
        eQr = (r["stored_ref"] + 2 + 2 * val) * EPS * r["sumsq_ref"]
    eQg = (r["stored"] + 2 + 2 * val) * EPS * r["sumsq"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mg, mr = r["means"], r["means_ref"]
        if lg:
            a, b = np.expm1(mg) + 1e-9, np.expm1(mr) + 1e-9
            da, db = np.exp(mg) * dmg + 9 * EPS * np.abs(a), np.exp(mr) * dmr + 9 * EPS * np.abs(b)
        else:
            a, b = mg + 1e-9, mr + 1e-9
            da, db = dmg + 9 * EPS * np.abs(a), dmr + 9 * EPS * np.abs(b)
        lfc = (da / np.abs(a) + db / np.abs(b) + EPS) / math.log(2.0) + 9 * EPS * np.abs(r["logfoldchanges"])
    out = {"means": dmg, "means_ref": dmr, "pct": 2 * EPS * r["pct"], "pct_ref": 2 * EPS * r["pct_ref"], "auc": 2 * EPS * np.abs(r["auc"]),
           "logfoldchanges": lfc}
    # the t-test's quantities
    with np.errstate(invalid="ignore", divide="ignore"):
        def var_term(n, m_, dm, Q, eQ):
            dss = eQ + n * (2 * np.abs(m_) * dm + 3 * EPS * m_ * m_) + EPS * Q
            v = np.maximum(Q - n * m_ * m_, 0) / np.maximum(n - 1, 1) / n
            return v, dss / (np.maximum(n - 1, 1) * n) + 3 * EPS * v

        va, dva = var_term(ng, mg, dmg, r["sumsq"], eQg)
        vb, dvb = var_term(nr, mr, dmr, r["sumsq_ref"], eQr)
        s = va + vb
        t = np.abs(r["scores"])
        out["t"] = (dmg + dmr + EPS * np.abs(mg - mr)) / np.sqrt(s) + t * ((dva + dvb) / (2 * s) + 4 * EPS)
        den = va * va / np.maximum(ng - 1, 1) + vb * vb / np.maximum(nr - 1, 1)
        out["df_rel"] = 2 * (dva + dvb) / s + (2 * va * dva / np.maximum(ng - 1, 1) + 2 * vb * dvb / np.maximum(nr - 1, 1)) / den + 8 * EPS
    return out


def _check_tables(rg, r, method, lg, rest, G, tag):
    print(f"{tag}:")
    b = _bounds(r, lg, rest, G)
    ratios = {}
    for k in ("means", "means_ref", "pct", "pct_ref", "auc"):
        ratios[k] = _ratio(k, rg[k], r[k], b[k])
    fin = np.isfinite(r["logfoldchanges"]) & np.isfinite(b["logfoldchanges"])
    assert np.array_equal(np.isfinite(rg["logfoldchanges"]), np.isfinite(r["logfoldchanges"]))
    ratios["logfoldchanges"] = _ratio("logfoldchanges", rg["logfoldchanges"], r["logfoldchanges"], b["logfoldchanges"], fin)
    live = ~np.isnan(r["scores"])
    if method == "wilcoxon":
        zb = 8 * EPS * np.abs(r["scores"])
        ratios["scores"] = _ratio("scores (z)", rg["scores"], r["scores"], zb)
        x = np.abs(r["scores"]) / math.sqrt(2.0)
        with np.errstate(invalid="ignore"):
            kappa = 2 * x / (math.sqrt(math.pi) * erfcx(x))
        pb = r["pvals"] * (10 * kappa + 16) * EPS + 2.0 ** -1000
        ratios["pvals"] = _ratio("pvals", rg["pvals"], r["pvals"], pb)
        sb = zb
    else:
        sb = np.where(live, b["t"], np.nan)
        some = live & (r["df"] > 0)
        assert np.array_equal(rg["scores"][live & ~some], r["scores"][live & ~some]) and (rg["pvals"][live & ~some] == 1).all()
        ratios["scores"] = _ratio("scores (t)", rg["scores"], r["scores"], sb, some)
        t, df = np.abs(r["scores"][some]), r["df"][some]
        dt, ddf = b["t"][some], b["df_rel"][some] * df
        p0 = r["pvals"][some]
        corners = [2 * tdist.sf(np.maximum(t + s1 * dt, 0), np.maximum(df + s2 * ddf, 1e-300)) for s1 in (-1, 1) for s2 in (-1, 1)]
        spread = np.max([np.abs(c - p0) for c in corners], axis=0)
        aa, bb, xx, yy = df / 2, 0.5, df / (df + t * t), t * t / (df + t * t)
        with np.errstate(divide="ignore", invalid="ignore"):                     # (t = 0: the library returns 1 without the prefactor)
            logs = np.where(yy > 0, np.abs(aa * np.log1p(-yy)) + np.abs(bb * np.log(np.where(yy > 0, yy, 1.0))), 0.0)
        pre = np.abs(gammaln(aa + bb)) + np.abs(gammaln(aa)) + abs(gammaln(bb)) + logs + 8
        pb = np.full(r["pvals"].shape, np.nan)
        direct = xx < (aa + 1) / (aa + bb + 2)
        pb[some] = spread + (np.where(direct, p0, 1 - p0) * 8 * pre + 32 * p0) * EPS + 2.0 ** -1000
        ratios["pvals"] = _ratio("pvals (t)", rg["pvals"], r["pvals"], pb, some)
    adj = np.stack([R.bh(rg["pvals"][g]) for g in range(G)])
    ratios["pvals_adj"] = _ratio("pvals_adj against bh(gpu pvals)", rg["pvals_adj"], adj, 4 * EPS * np.abs(adj))
    margin = R.score_margin(r["scores"], np.where(live, sb, 0.0))
    print(f"  order: the reference's smallest score gap is {margin:.3g} x the bounds")
    assert np.array_equal(rg["order"], r["order"])
    assert np.array_equal(rg["group_sizes"], r["sizes"])
    return ratios


# ---- the stage entry: bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref", [("counts1025", -1), ("counts1025", 3), ("raw3001", -1), ("raw3001", 2), ("raw3001", 0), ("two1025", -1),
                                      ("two1025", 1), ("pairs2048", -1), ("pairs2048", 5)])
def test_rank_sums_bit_for_bit(sa, cases, name, ref):
    from sharp_amd import rank_genes

    X, codes, G, opt = cases[name]
    r = _ref(cases, name, ref=ref)
    r2, ties, cnt = rank_genes._rank_sums(X, codes, G, reference=ref, **opt)
    rows = np.arange(G) != ref
    assert np.array_equal(r2[rows], r["rank2"][rows]) and np.array_equal(cnt[rows], r["nz"][rows])
    if ref < 0:
        assert np.array_equal(ties, r["ties"][0])
    else:
        assert np.array_equal(ties[rows], r["ties"][rows])
        assert (r2[ref] == -7).all() and (ties[ref] == -7).all() and (cnt[ref] == -7).all()          # the caller's fill is left alone


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method,ref", [("counts1025", "wilcoxon", -1), ("counts1025", "wilcoxon", 3), ("counts1025", "t-test", -1),
                                             ("counts1025", "t-test", 3), ("raw3001", "wilcoxon", -1), ("raw3001", "wilcoxon", 2),
                                             ("two1025", "wilcoxon", -1), ("two1025", "t-test", 1), ("two1025", "t-test", -1),
                                             ("pairs2048", "wilcoxon", -1), ("pairs2048", "wilcoxon", 5), ("pairs2048", "t-test", 5)])
def test_tables(sa, cases, name, method, ref):
    X, codes, G, opt = cases[name]
    r = _ref(cases, name, method, ref)
    rg = _call(sa, cases, name, method, ref)
    _check_tables(rg, r, method, 1 if opt["log1p"] else 0, ref < 0, G, f"{name} {method} reference {ref}")
    if ref >= 0:
        for k in ("scores", "pvals", "pvals_adj", "logfoldchanges", "auc", "means", "means_ref", "pct", "pct_ref"):
            assert np.isnan(rg[k][ref]).all()
        assert np.array_equal(rg["order"][ref], np.arange(X.shape[0]))
    if name in ("raw3001", "two1025") and method == "wilcoxon":
        others = np.arange(G) != ref
        assert (rg["scores"][others, 2] == 0).all() and (rg["pvals"][others, 2] == 1).all()            # sigma = 0: every value tied


@pytest.mark.parametrize("tie_correct,continuity", [(False, False), (True, True), (False, True)])
def test_tie_correct_and_continuity(sa, cases, tie_correct, continuity):
    for name, ref in (("counts1025", -1), ("two1025", 0)):
        X, codes, G, opt = cases[name]
        r = _ref(cases, name, "wilcoxon", ref, tie_correct=tie_correct, continuity=continuity)
        rg = _call(sa, cases, name, "wilcoxon", ref, tie_correct=tie_correct, continuity=continuity)
        _check_tables(rg, r, "wilcoxon", 1 if opt["log1p"] else 0, ref < 0, G, f"{name} tie_correct {tie_correct} continuity {continuity}")
    assert rg["tie_correct"] == tie_correct and rg["continuity"] == continuity


_KEYS = ("scores", "pvals", "pvals_adj", "logfoldchanges", "auc", "means", "means_ref", "pct", "pct_ref", "order", "group_sizes")


def _same_bits(a, b, rows=None):
    for k in _KEYS:
        x, y = a[k], b[k]
        if rows is not None and k not in ("order", "group_sizes"):
            y = y[:, rows]
        if rows is not None and k == "order":
            continue
        assert x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("method,ref", [("wilcoxon", -1), ("t-test", 3)])
def test_blocks_and_repeats_give_the_same_bits(sa, cases, method, ref):
    X, codes, G, opt = cases["counts1025"]
    one = _call(sa, cases, "counts1025", method, ref)
    _same_bits(one, _call(sa, cases, "counts1025", method, ref))
    blocks = E.ragged(X, [1, 700])
    assert [b.shape[1] for b in blocks] == [1, 699, 325]
    _same_bits(one, _call(sa, cases, "counts1025", method, ref, blocks=blocks))


def test_gene_subset_is_the_full_calls_rows(sa, cases):
    X, codes, G, opt = cases["counts1025"]
    keep = np.array([0, 1, 3, 17, 64, 65, 130, 198])
    full = _call(sa, cases, "counts1025")
    sub = _call(sa, cases, "counts1025", genes=keep, n_genes=5)
    for k in ("scores", "pvals", "logfoldchanges", "auc", "means", "means_ref", "pct", "pct_ref"):
        assert sub[k].tobytes() == np.ascontiguousarray(full[k][:, keep]).tobytes(), k          # normalisation ran over all genes
    assert sub["order"].shape == (G, 5) and np.array_equal(sub["order"], R.order_of(sub["scores"])[:, :5])
    assert np.array_equal(sub["pvals_adj"], np.stack([R.bh(sub["pvals"][g]) for g in range(G)])) or np.allclose(
        sub["pvals_adj"], np.stack([R.bh(sub["pvals"][g]) for g in range(G)]), rtol=4 * EPS, atol=0)
    assert np.array_equal(sub["genes"], keep) and full["genes"] is None


def test_labels_of_any_kind(sa, cases):
    X, codes, G, opt = cases["two1025"]
    names = np.array(["b", "a"])[codes]                       # np.unique orders them: "a" is code 0
    a = sa.rank_genes_groups(X, names, reference="a", **opt)
    b = sa.rank_genes_groups(X, 1 - codes, reference=0, **opt)
    _same_bits(a, b)
    assert a["groups"].tolist() == ["a", "b"] and a["reference"] == "a" and a["method"] == "wilcoxon"


def test_auc_is_get_marker_genes_auroc(sa, cases):
    X, codes = R.raw_case(1025, 40, 4, 2, 512)
    A = X.toarray()
    assert np.array_equal(A.astype(np.float32).astype(np.float64), A)
    rg = sa.rank_genes_groups(X, codes, normalize_total=None, log1p=False)
    mk = sa.get_marker_genes(A, codes + 1, theta=0.0, ng=4)["gallinfo"]
    genes, auroc, ic = mk["gene"], mk["auc"], mk["icluster"] - 1
    assert genes.size >= 38
    n = codes.size
    n1 = np.bincount(codes)[ic].astype(float)
    bound = 8 * EPS * (1 + (n1 + 1) / (2 * (n - n1))) + 2 * EPS
    d = np.abs(rg["auc"][:, genes].max(0) - auroc)
    print(f"auc against get_marker_genes: largest difference {d.max():.3e}, largest ratio to its bound {(d / bound).max():.3f}")
    assert (d <= bound).all()


def test_planted_genes_head_their_group(sa):
    X, codes, G = R.planted_case()
    rg = sa.rank_genes_groups(X, codes)
    m = X.shape[0]
    for g in range(G):
        mine = set(np.arange(g, m, G).tolist())
        assert set(rg["order"][g, :len(mine)].tolist()) == mine


def test_refusals(sa, cases):
    from sharp_amd import rank_genes

    X, codes, G, opt = cases["two1025"]
    n = codes.size
    with pytest.raises(sa.SharpError, match="at least 2 groups"):
        sa.rank_genes_groups(X, np.zeros(n, int), **opt)
    with pytest.raises(sa.SharpError, match="rank_sums: need at least 2 groups"):
        rank_genes._rank_sums(X, np.zeros(n, np.int32), 1, **opt)
    with pytest.raises(sa.SharpError, match="group 2 .counted from 0. has no cell"):
        rank_genes._rank_sums(X, codes, 3, **opt)                                # a code that no cell carries
    with pytest.raises(sa.SharpError, match="rank_sums: at most 1024 groups"):
        rank_genes._rank_sums(X, np.arange(n, dtype=np.int32) % 1025, 1025, **opt)
    with pytest.raises(sa.SharpError, match="labels must be codes"):
        rank_genes._rank_sums(X, codes + 1, 2, **opt)
    with pytest.raises(sa.SharpError, match="reference must be -1"):
        rank_genes._rank_sums(X, codes, 2, reference=2, **opt)
    with pytest.raises(sa.SharpError, match="one label per cell"):
        sa.rank_genes_groups(X, codes[:-1], **opt)
    with pytest.raises(sa.SharpError, match="reference must be"):
        sa.rank_genes_groups(X, codes, reference=7, **opt)
    one = codes.copy()
    one[:] = 0
    one[0] = 1
    with pytest.raises(sa.SharpError, match="t-test needs at least 2 cells"):
        sa.rank_genes_groups(X, one, method="t-test", **opt)
    with pytest.raises(sa.SharpError, match="method must be"):
        sa.rank_genes_groups(X, codes, method="logreg", **opt)
    r = sa.rank_genes_groups(X, one, **opt)                                      # a group of a single cell is fine for Wilcoxon
    assert r["group_sizes"].tolist() == [n - 1, 1]
