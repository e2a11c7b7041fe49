"""tests/_prepare_ref.py checked on the CPU: what tests/test_prepare_gpu.py rests on holds without a GPU."""
import numpy as np
import pytest

import _prepare_ref as ref
import _tsne_ref as tref

LD = np.longdouble


@pytest.mark.parametrize("center,scale", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_sliced_gram_is_the_longdouble_gram(center, scale):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(700, 33)) * 10.0 ** rng.uniform(-3, 3, 33) + 5.0
    Xc, _, _ = ref.centre_scale(X, center, scale)
    Gs, Gd = ref.gram_sliced(Xc), ref.gram_direct(Xc)
    top = np.sqrt(np.outer(np.diag(Gd), np.diag(Gd)))
    # the direct product rounds every one of its n additions to 64 bits; the sliced one is exact up to what the slices drop
    assert float((np.abs(Gs - Gd) / top).max()) <= 700 * 2.0 ** -64


def test_reference_agrees_with_the_fp64_statement():
    X = ref.spectrum_data(300, 12, 8, seed=3)
    for center in (True, False):
        for scale in (True, False):
            R = ref.pca(X, 6, center, scale)
            want, V = tref.pca(X, 6, center, scale)
            assert np.abs(R["scores"].astype(np.float64) - want).max() <= 1e-9 * np.abs(want).max()
            assert np.abs(R["V"] - V).max() <= 1e-9
    assert ref.relative_gaps(ref.pca(X, 6)["w"], 6).min() >= 0.05


def test_sign_rule_and_divisors():
    V = np.array([[0.1, -0.2], [-0.9, 0.5], [0.3, -0.6]])
    S = ref.sign_rule(V)
    assert np.array_equal(S[:, 0], -V[:, 0]) and np.array_equal(S[:, 1], -V[:, 1])
    X = np.array([[1.0, 2.0], [3.0, 2.0], [5.0, 8.0]])
    _, mu, sd = ref.centre_scale(X, True, True)
    assert np.array_equal(mu, [3.0, 4.0]) and np.allclose(sd.astype(float), [2.0, np.sqrt(12.0)])
    _, mu, sd = ref.centre_scale(X, False, True)                    # the root mean square about zero, divisor n - 1
    assert not mu.any() and np.allclose(sd.astype(float), [np.sqrt(35 / 2), np.sqrt(72 / 2)])


@pytest.mark.parametrize("n,d", [(2, 1), (3, 1), (513, 17), (1023, 257), (33001, 5)])
def test_design_properties(n, d):
    for offsets in (True, False):
        X, o = ref.design(n, d, offsets)
        Xc, dg = ref.check_design(X, o, center=offsets)
        k = min(d, max(1, n // 2))
        want = ref.design_expected(Xc, dg, k)
        assert want.shape == (n, min(k, d)) and np.array_equal(want.sum(0), np.zeros(want.shape[1]))
    D = ref.dense_pairs(n, d, 1)
    assert not D.sum(0).any() and np.array_equal(D, np.rint(D))
