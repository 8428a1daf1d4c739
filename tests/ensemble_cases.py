"""Crafted probabilities for the ensemble averaging (tests/test_ensemble.py on the host twin, tests/test_ensemble_gpu.py on the kernel)
and the yardstick both are measured against: the reference's text path itself -- '{:0.6f}' of every float32, float() of the digits,
the sum in input order and the division in double, '{:.6f}' of the mean, float32 of those digits (clair/call_var.py:950-1000,
clair/post_processing/ensemble.py:33-43 and :67, clair/call_var.py:1291).  Never the rule under test."""
import numpy as np

MILLION = 1000000


def float_values(n=120000, seed=1):
    """float32 values in [0, 1]: uniform ones, softmax-sized small ones, float32((i + 0.5) / 1e6) and its float32 neighbours, and the
    64 values (2j + 1) * 15625 / 2e6 that ARE exact half-way points in binary (2e6 = 2^7 * 5^6), where the tie rule decides."""
    rng = np.random.default_rng(seed)
    i = rng.integers(0, MILLION, n // 4)
    half = ((i + 0.5) / 1e6).astype(np.float32)
    exact = ((2 * np.arange(64) + 1) * 15625 / 2e6).astype(np.float32)
    assert np.array_equal(exact.astype(np.float64) * 2e6, (2 * np.arange(64) + 1) * 15625.0)
    parts = [rng.random(n // 4, dtype=np.float32), (rng.random(n // 4) ** 8).astype(np.float32), half,
             np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), exact,
             np.array([0.0, 1.0, 1e-7, 4.9e-7, 5e-7, 5.1e-7, 0.9999995, 0.99999949], dtype=np.float32)]
    return np.concatenate(parts)


def crafted_rows(models, n, seed=2):
    """float32 [models, n]: one value per model and case.  The first half of the cases (for an even number of models) are built so
    that the six-decimal values sum to K/2 modulo K -- the true mean lies EXACTLY half-way between two six-decimal numbers, where the
    double a = s / K is a hair above or below it, or on it; the rest are independent values, a third of them softmax-small."""
    rng = np.random.default_rng(seed + 1000 * models)
    k = rng.integers(0, MILLION - models, (models, n))
    small = rng.random(n) < 1.0 / 3.0
    k[:, small] = rng.integers(0, 60, (models, int(small.sum())))
    if models % 2 == 0:
        h = n // 2 + 1
        k[-1, :h] += (models // 2 - k[:, :h].sum(axis=0)) % models
        assert ((k[:, :h].sum(axis=0) % models) == models // 2).all()
    p = (k / 1e6).astype(np.float32)
    assert np.array_equal(np.rint(p.astype(np.float64) * 1e6).astype(np.int64), k)      # float32 keeps six decimals below 1
    return p


def text_of(p):
    """'{:0.6f}'.format(v) for every float32 v (the float64 of a float32 is exact, so '%.6f' of it prints the same digits)."""
    return ["%.6f" % v for v in np.asarray(p, dtype=np.float32).ravel().tolist()]


def text_average(P):
    """The yardstick: P float32 [K, n] -> float32 [n] through the text path."""
    P = np.asarray(P, dtype=np.float32)
    models, n = P.shape
    digits = [text_of(P[j]) for j in range(models)]
    out = []
    for i in range(n):
        s = float(digits[0][i])
        for j in range(1, models):
            s = s + float(digits[j][i])
        out.append("{:.6f}".format(s / models))
    return np.array(out, dtype=np.float32)


def naive_average(P):
    """What the rule must NOT be: the mean's rounded product with 1e6, then rint."""
    P = np.asarray(P, dtype=np.float32)
    d = np.rint(P.astype(np.float64) * 1e6) / 1e6
    s = d[0].copy()
    for j in range(1, P.shape[0]):
        s = s + d[j]
    return (np.rint((s / P.shape[0]) * 1e6) / 1e6).astype(np.float32)
