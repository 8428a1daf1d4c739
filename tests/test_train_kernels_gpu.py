"""The training path's own kernels on the MI355X, one launch at a time: tgemm (csrc/train_gemm.hip.h) and column_sum_kernel
(csrc/train_kernels.hip.h) through clair_train_debug_gemm / clair_train_debug_column_sum, the loss kernel at its clips through a network whose
logits the host knows bit for bit, and the default micro-batch of 1 024 rows whole against the same rows in 16 pieces (docs/train.md).

Exact tests: every operand holds small integers (A, B, x in -2 .. 2, bias and the initial C / out in -8 .. 8), so every product and every
partial sum is an integer below 2^24 in magnitude and float32 holds it exactly, whatever order the kernel adds in: the result must EQUAL the
integer product.  The arrays handed to the device carry sentinels (12 345.0 and up) in every element the launch does not address, between
the rows, columns and batches and behind the last one; they must come back as they went.

Rounding tests: standard-normal operands at the shapes of the default micro-batch against float64, under the a-priori bound of a float32 sum
of K terms in any order, gamma_K * sum |terms|, and -- as a Frobenius norm -- within 4 times the error of a NumPy float32 stand-in that adds in
the kernel's documented order.  The first is a condition and the second a margin reasoned in docs/train.md; neither is a measurement.
"""
import os
import sys

import numpy as np
import pytest
import torch

from clair_amd import _capi, synth, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_num_threads(4)
EPS32 = float(np.finfo(np.float32).eps)
U32 = 2.0 ** -24                                   # unit roundoff of float32
T_STEPS = 33
HEAD_OFF, HEAD_SIZE = (0, 21, 24, 57), (21, 3, 33, 33)
SENTINEL = 12345.0
NO_DROPOUT = (0.0,) * 6
STRIDE_NAMES = ("sam", "sak", "sbk", "sbn", "scm", "scn", "ba", "bb", "bc", "bbias")


@pytest.fixture(scope="module")
def trainer():
    t = _capi.Trainer(0, 8, "Adam", "FocalLoss")
    yield t
    t.close()


def gamma(k):
    return k * U32 / (1.0 - k * U32)


# ---- tgemm ------------------------------------------------------------------------------------------------------------------------------
def _gemm(M, N, K, strides, batch=1, accumulate=0, bias=False):
    s = dict(zip(STRIDE_NAMES, strides))
    return dict(M=M, N=N, K=K, batch=batch, accumulate=accumulate, bias=bias, **s)


def _laid_out(M, N, K, a="k", b="n", scn=1, batch=1, accumulate=0, bias=False, shared=None):
    """A hand-picked case.  a: "k" (sak == 1), "m" (sam == 1) or "x" (neither); b: "n" (sbn == 1), "k" (sbk == 1) or "x"; rows, columns and
    batches are spaced wider than they need to be, so sentinels lie between them; shared: the operand whose batch stride is 0."""
    sam, sak = {"k": (K + 3, 1), "m": (1, M + 2), "x": (2 * K + 1, 2)}[a]
    sbk, sbn = {"n": (N + 1, 1), "k": (1, K + 2), "x": (3 * N + 2, 3)}[b]
    scm = N * scn + 4
    ba = 0 if shared == "a" else (M - 1) * sam + (K - 1) * sak + 6
    bb = 0 if shared == "b" else (K - 1) * sbk + (N - 1) * sbn + 4
    bc = (M - 1) * scm + (N - 1) * scn + 10
    return _gemm(M, N, K, (sam, sak, sbk, sbn, scm, scn, ba, bb, bc, N + 2), batch, accumulate, bias)


def _view(flat, extents, strides):
    """the operand inside its flat array, [extent0, extent1, extent2], without a copy; the callers size `flat` by _span"""
    assert flat.ndim == 1 and _span(extents, strides) <= flat.size and min(strides) >= 0
    return np.lib.stride_tricks.as_strided(flat, shape=extents, strides=[s * flat.itemsize for s in strides])


def _span(extents, strides):
    """the largest element index of an operand, plus one"""
    return sum((e - 1) * s for e, s in zip(extents, strides)) + 1


def _shapes(g):
    """extents and strides of A [batch, M, K], B [batch, K, N], C [batch, M, N] and bias [batch, 1, N]"""
    return (((g["batch"], g["M"], g["K"]), (g["ba"], g["sam"], g["sak"])), ((g["batch"], g["K"], g["N"]), (g["bb"], g["sbk"], g["sbn"])),
            ((g["batch"], g["M"], g["N"]), (g["bc"], g["scm"], g["scn"])), ((g["batch"], 1, g["N"]), (g["bbias"], 0, 1)))


def _operands(g, draw_a, draw_b, draw_c, draw_bias, margin=67):
    """-> flat a, b, c0, bias (or None): draw_*(shape) gives the values of the addressed elements, everything else is a sentinel"""
    out = []
    for (extents, strides), draw in zip(_shapes(g), (draw_a, draw_b, draw_c, draw_bias)):
        flat = (SENTINEL + np.arange(_span(extents, strides) + margin) % 7).astype(np.float32)
        _view(flat, extents, strides)[...] = draw(extents)
        out.append(flat)
    a, b, c0, bias = out
    probe = np.zeros(c0.size, dtype=np.int64)                      # no two elements of C may share an address
    numbered = np.arange(g["batch"] * g["M"] * g["N"]).reshape(g["batch"], g["M"], g["N"])
    _view(probe, *_shapes(g)[2])[...] = numbered
    assert np.array_equal(_view(probe, *_shapes(g)[2]), numbered), "the case lets two elements of C share an address"
    return a, b, c0, (bias if g["bias"] else None)


def _launch(t, g, a, b, c0, bias):
    dims = [g[k] for k in ("M", "N", "K", "batch", "accumulate")]
    return t.debug_gemm(a, b, c0, dims, [g[k] for k in STRIDE_NAMES], bias)


def _integer_product(A, B):
    """The int64 product "bmk,bkn->bmn" of integer-valued arrays.  Small products are an int64 einsum as it stands; the large ones go through the
    float64 BLAS, which gives the same integers bit for bit: every partial sum is an integer below 2^53, so no order of addition rounds."""
    if A.shape[0] * A.shape[1] * A.shape[2] * B.shape[2] <= 1 << 22:
        return np.einsum("bmk,bkn->bmn", A.astype(np.int64), B.astype(np.int64))
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    assert np.array_equal(A64, np.rint(A64)) and np.array_equal(B64, np.rint(B64))
    assert float(np.abs(A64).max()) * float(np.abs(B64).max()) * A.shape[2] < 2.0 ** 53
    return np.matmul(A64, B64).astype(np.int64)


def _check_exact(t, g, seed):
    rng = np.random.default_rng(seed)
    small = lambda shape: rng.integers(-2, 3, shape).astype(np.float32)        # noqa: E731
    wide = lambda shape: rng.integers(-8, 9, shape).astype(np.float32)         # noqa: E731
    a, b, c0, bias = _operands(g, small, small, wide, wide)
    sa, sb, sc, sbias = _shapes(g)
    got = _launch(t, g, a, b, c0, bias)
    want = _integer_product(_view(a, *sa), _view(b, *sb))
    if bias is not None:
        want = want + _view(bias, *sbias).astype(np.int64)
    if g["accumulate"]:
        want = want + _view(c0, *sc).astype(np.int64)
    assert np.abs(want).max() < 1 << 24
    expected, untouched = c0.copy(), np.ones(c0.size, dtype=bool)
    _view(expected, *sc)[...] = want.astype(np.float32)
    _view(untouched, *sc)[...] = False
    assert got.shape == c0.shape
    wrong = np.argwhere(_view(got, *sc) != _view(expected, *sc))
    assert len(wrong) == 0, "%d of %d elements of C differ, the first at (batch, m, n) = %r: got %r, want %r" % (
        len(wrong), want.size, tuple(wrong[0]), _view(got, *sc)[tuple(wrong[0])], want[tuple(wrong[0])])
    assert np.array_equal(got[untouched], c0[untouched]), "an element of C outside M x N x batch was written"
    assert np.array_equal(got, expected)


# the edges of the 64 x 64 block, the 32 x 32 wave tile and the 16-wide K slab; every layout of A and B; C with scn != 1 and a ragged N block;
# batch 1, 4, 256, a batch stride of 0, bbias; bias and accumulate alone and together
HAND_PICKED = [
    dict(M=1, N=1, K=1),
    dict(M=31, N=3, K=2, a="m", bias=True),
    dict(M=32, N=21, K=15, b="k", accumulate=1),
    dict(M=33, N=33, K=16, a="x", bias=True, accumulate=1),
    dict(M=63, N=63, K=17, b="x"),
    dict(M=64, N=64, K=33, a="m", b="k", bias=True),
    dict(M=65, N=65, K=96, a="x", b="x", accumulate=1),
    dict(M=130, N=96, K=33, bias=True, accumulate=1),
    dict(M=32, N=32, K=16),
    dict(M=64, N=64, K=16, a="m"),
    dict(M=130, N=21, K=17, a="m", scn=5),
    dict(M=63, N=65, K=1, a="x", scn=2, bias=True, accumulate=1),
    dict(M=33, N=63, K=15, b="k", scn=256, accumulate=1),
    dict(M=65, N=33, K=15, scn=3, batch=4, bias=True),
    dict(M=33, N=65, K=16, a="m", b="x", batch=4, accumulate=1, shared="b"),
    dict(M=65, N=63, K=2, b="x", batch=4, bias=True, accumulate=1),
    dict(M=64, N=96, K=17, a="x", b="k", batch=4, shared="a"),
    dict(M=31, N=3, K=96, a="x", b="k", batch=256, bias=True),
    dict(M=1, N=96, K=33, batch=256, accumulate=1, shared="a"),
    dict(M=33, N=21, K=2, a="m", scn=2, batch=256, bias=True, accumulate=1, shared="b"),
    dict(M=64, N=1, K=1, bias=True),
    dict(M=1, N=64, K=2, a="m", b="k"),
    dict(M=130, N=1, K=33, a="m", b="x", accumulate=1),
    dict(M=1, N=65, K=96, a="x", bias=True),
    dict(M=31, N=33, K=17, b="k", bias=True),
    dict(M=63, N=3, K=16, a="x", b="k", accumulate=1),
    dict(M=32, N=64, K=1, a="m", bias=True, accumulate=1),
    dict(M=65, N=21, K=33, b="x", scn=7, bias=True),
]


def _case_id(c):
    return "-".join("%s%s" % (k, v) for k, v in c.items())


@pytest.mark.parametrize("case", HAND_PICKED, ids=_case_id)
def test_tgemm_exact_edges_and_layouts(trainer, case):
    _check_exact(trainer, _laid_out(**case), seed=sum(case[k] for k in "MNK"))


def trainer_call_sites(n):
    """Every gemm(...) of csrc/train.hip with the arguments a micro-batch of n rows gives it: (call site, case)"""
    T, HID = T_STEPS, 128
    sites = []
    for layer, width in ((1, 32), (2, 256)):
        sites += [
            ("lstm_forward layer %d: x projection of all steps" % layer, _gemm(T * n, 512, width, (width, 1, 512, 1, 512, 1, 0, 0, 0, 0), bias=True)),
            ("lstm_backward layer %d: dK_x += X^T . dz" % layer, _gemm(width, 512, T * n, (1, width, 512, 1, 512, 1, 0, 0, 0, 0), accumulate=1)),
        ]
    sites += [
        ("lstm_forward: z_t += h_prev . K_h", _gemm(n, 512, HID, (256, 1, 512, 1, 512, 1, 0, 0, 0, 0), accumulate=1)),
        ("lstm_backward: dhrec = dz_t . K_h^T", _gemm(n, HID, 512, (512, 1, 1, 512, HID, 1, 0, 0, 0, 0))),
        ("lstm_backward: dK_h += h_prev^T . dz_next", _gemm(HID, 512, (T - 1) * n, (1, 256, 512, 1, 512, 1, 0, 0, 0, 0), accumulate=1)),
        ("lstm_backward layer 2: dX = dz . K_x^T, forward direction", _gemm(T * n, 256, 512, (512, 1, 1, 512, 256, 1, 0, 0, 0, 0))),
        ("lstm_backward layer 2: dX += dz . K_x^T, backward direction", _gemm(T * n, 256, 512, (512, 1, 1, 512, 256, 1, 0, 0, 0, 0), accumulate=1)),
        ("L3 forward, batch of 256 channels", _gemm(n, 30, T, (256, n * 256, 30, 1, 7680, 256, 1, T * 30, 1, 30), batch=256, bias=True)),
        ("L4 forward", _gemm(n, 192, 7680, (7680, 1, 192, 1, 192, 1, 0, 0, 0, 0), bias=True)),
        ("L5 forward, batch of 4 on one shared d4", _gemm(n, 96, 192, (192, 1, 96, 1, 96, 1, 0, 192 * 96, n * 96, 96), batch=4, bias=True)),
        ("L5 backward: dW5_k += d4^T . dd5_k", _gemm(192, 96, n, (1, 192, 96, 1, 96, 1, 0, 0, 0, 0), accumulate=1)),
        ("L5 backward: dd4 = dd5_0 . W5_0^T", _gemm(n, 192, 96, (96, 1, 1, 96, 192, 1, 0, 0, 0, 0))),
        ("L5 backward: dd4 += dd5_k . W5_k^T", _gemm(n, 192, 96, (96, 1, 1, 96, 192, 1, 0, 0, 0, 0), accumulate=1)),
        ("L4 backward: dW4 += l3^T . dd4", _gemm(7680, 192, n, (1, 7680, 192, 1, 192, 1, 0, 0, 0, 0), accumulate=1)),
        ("L4 backward: dl3 = dd4 . W4^T", _gemm(n, 7680, 192, (192, 1, 1, 192, 7680, 1, 0, 0, 0, 0))),
        ("L3 backward: dW3 += a2d^T . dz3, batch of 256", _gemm(T, 30, n, (n * 256, 256, 7680, 256, 30, 1, 1, 1, T * 30, 0), batch=256, accumulate=1)),
        ("L3 backward: da2 = dz3 . W3^T, batch of 256", _gemm(n, T, 30, (7680, 256, 1, 30, 256, n * 256, 1, T * 30, 1, 0), batch=256)),
    ]
    for size in (21, 3, 33):
        sites += [
            ("head of %d forward" % size, _gemm(n, size, 96, (96, 1, size, 1, 90, 1, 0, 0, 0, 0), bias=True)),
            ("head of %d backward: dW += d5^T . dz" % size, _gemm(96, size, n, (1, 96, 90, 1, size, 1, 0, 0, 0, 0), accumulate=1)),
            ("head of %d backward: dd5 = dz . W^T" % size, _gemm(n, 96, size, (90, 1, 1, size, 96, 1, 0, 0, 0, 0))),
        ]
    return sites


@pytest.mark.parametrize("site,case", trainer_call_sites(65), ids=[s for s, _ in trainer_call_sites(65)])
def test_tgemm_exact_at_the_trainers_arguments(trainer, site, case):
    """n = 65: a last row block of one row, K up to 33 * 65 = 2 145"""
    _check_exact(trainer, case, seed=len(site))


def test_tgemm_exact_at_k_33792(trainer):
    """dK_h of the default micro-batch in the trainer's own layout (h_prev inside rows of 256, m fast): 2 112 K slabs"""
    _check_exact(trainer, _gemm(128, 512, 33 * 1024, (1, 256, 512, 1, 512, 1, 0, 0, 0, 0), accumulate=1), seed=3)


def _sequential_float32(a, b):
    """the stand-in of tgemm's order: a [K, m], b [K, n] float32 -> [m, n], the K products added one at a time in ascending k, each product and
    each sum rounded to float32"""
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[0]):
        acc += a[k][:, None] * b[k][None, :]
    return acc


@pytest.mark.parametrize("M,N,K", [(128, 512, 32 * 1024), (32, 512, 33 * 1024), (256, 512, 33 * 1024)], ids=["dK_h", "lstm1_dK_x", "lstm2_dK_x"])
def test_tgemm_rounding_at_the_default_micro_batch(trainer, M, N, K):
    """the three weight-gradient shapes at n = 1 024, A m-fast and B n-fast as the trainer has them"""
    rng = np.random.default_rng(K + M)
    a = rng.standard_normal((K, M)).astype(np.float32)           # A(m, k) = a[k * M + m]
    b = rng.standard_normal((K, N)).astype(np.float32)
    got = trainer.debug_gemm(a, b, np.zeros(M * N, dtype=np.float32), (M, N, K, 1, 0), (1, M, N, 1, N, 1, 0, 0, 0, 0)).reshape(M, N)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    want = a64.T @ b64
    S = np.abs(a64).T @ np.abs(b64)
    err = np.abs(got.astype(np.float64) - want)
    print("tgemm M=%d N=%d K=%d: worst |C - C64| / (gamma_K S) = %.3g" % (M, N, K, float((err / (gamma(K) * S)).max())))
    corner = (slice(0, 32), slice(0, 32))
    frobenius = lambda c: float(np.linalg.norm(c.astype(np.float64) - want[corner]) / np.linalg.norm(S[corner]))      # noqa: E731
    device, stand_in, blas = frobenius(got[corner]), frobenius(_sequential_float32(a[:, :32], b[:, :32])), frobenius(a[:, :32].T @ b[:, :32])
    print("tgemm M=%d N=%d K=%d, 32x32 corner: device %.3g, sequential float32 stand-in %.3g, BLAS float32 %.3g of ||S||; device / stand-in %.3g, "
          "device / BLAS %.3g" % (M, N, K, device, stand_in, blas, device / stand_in, device / blas))
    assert (err <= gamma(K) * S).all()
    assert device <= 4 * stand_in


# ---- column_sum_kernel --------------------------------------------------------------------------------------------------------------------
def _column_sum_case(t, rng, rows, cols, ld, d=1, s1=1, s2=0, offset=0, margin=41):
    """x is a [rows, ld] matrix whose columns offset .. offset + cols are summed; the device is handed the matrix from `offset` on"""
    x = rng.integers(-2, 3, rows * ld).astype(np.float32)
    j = np.arange(cols)
    target = (j // d) * s1 + (j % d) * s2
    assert np.unique(target).size == cols
    out = SENTINEL + (np.arange(int(target.max()) + 1 + margin) % 7).astype(np.float32)
    out[target] = rng.integers(-8, 9, cols).astype(np.float32)
    got = t.debug_column_sum(x[offset:], rows, cols, ld, out, d, s1, s2)
    expected = out.copy()
    expected[target] = (out[target].astype(np.int64) + x.reshape(rows, ld)[:, offset:offset + cols].astype(np.int64).sum(axis=0)).astype(np.float32)
    assert np.abs(expected[target]).max() < 1 << 24
    assert np.array_equal(got, expected), (rows, cols, ld, d, s1, s2, offset)


COLUMN_SUMS = [
    # rows, cols, ld
    (1, 1, 1), (7, 3, 3), (8, 21, 21), (9, 31, 31), (64, 32, 32), (2145, 33, 33), (2145, 96, 96), (33792, 512, 512), (33792, 1, 1),
    (1, 512, 512), (7, 33, 40), (9, 96, 97), (64, 31, 512), (8, 3, 90), (2145, 21, 90), (65, 32, 33),
]


@pytest.mark.parametrize("rows,cols,ld", COLUMN_SUMS)
def test_column_sum_exact(trainer, rows, cols, ld):
    _column_sum_case(trainer, np.random.default_rng(rows + cols), rows, cols, ld)


@pytest.mark.parametrize("head", range(4))
def test_column_sum_exact_at_a_column_offset(trainer, head):
    """the heads' bias gradients: dz + HEAD_OFF[k], ld = 90"""
    _column_sum_case(trainer, np.random.default_rng(head), 65, HEAD_SIZE[head], 90, offset=HEAD_OFF[head])


@pytest.mark.parametrize("rows,cols,ld,d,s1,s2", [(65, 7680, 7680, 256, 1, 30), (9, 33, 35, 1, 2, 0), (64, 96, 96, 32, 40, 1), (7, 21, 21, 4, 1, 11)],
                         ids=["l3_bias", "every_other", "blocks_of_32", "transposed"])
def test_column_sum_exact_scattered(trainer, rows, cols, ld, d, s1, s2):
    """(d, s1, s2): L3's bias gradient (256, 1, 30) -- column u * 256 + c to [c][u] -- and scatters that leave sentinels between the sums"""
    _column_sum_case(trainer, np.random.default_rng(cols), rows, cols, ld, d, s1, s2)


def test_column_sum_rounding_at_the_default_micro_batch(trainer):
    """the LSTM bias gradients of 1 024 rows: 33 792 rows of 512 columns"""
    rows, cols = 33 * 1024, 512
    x = np.random.default_rng(5).standard_normal((rows, cols)).astype(np.float32)
    got = trainer.debug_column_sum(x, rows, cols, cols, np.zeros(cols, dtype=np.float32)).astype(np.float64)
    x64 = x.astype(np.float64)
    want, S = x64.sum(axis=0), np.abs(x64).sum(axis=0)
    partial = np.zeros((8, cols), dtype=np.float32)                 # the kernel's stated order: 8 strided sequential partials, then 8 adds
    for r in range(0, rows, 8):
        partial += x[r:r + 8]
    total = partial[0].copy()
    for k in range(1, 8):
        total += partial[k]
    total = np.zeros(cols, dtype=np.float32) + total
    device, stand_in = (float(np.linalg.norm(v - want) / np.linalg.norm(S)) for v in (got, total.astype(np.float64)))
    print("column_sum rows=%d cols=%d: worst |s - s64| / (gamma_rows sum|x|) = %.3g; device %.3g, stand-in %.3g of ||sum|x|||, device / stand-in %.3g, "
          "%d of %d sums equal the stand-in's bits" % (rows, cols, float((np.abs(got - want) / (gamma(rows) * S)).max()), device, stand_in, device / stand_in,
                                                        int((got == total).sum()), cols))
    assert (np.abs(got - want) <= gamma(rows) * S).all()
    assert device <= 4 * stand_in


# ---- the loss kernel at its clips -----------------------------------------------------------------------------------------------------------
SELU_SCALE32 = np.float32(R.SELU_SCALE)


def _loss_weights(head_biases):
    """fresh weights with the four head kernels zero: every row's SELU'd logits are float32(SELU_SCALE) * bias, whatever the input"""
    w = dict(weights.synthetic_weights())
    for (name, _, size), bias in zip(R.HEADS, head_biases):
        assert bias.shape == (size,) and bias.dtype == np.float32 and (bias > 0).all()      # clear of SELU's kink at zero
        w["head_%s_kernel" % name] = np.zeros_like(w["head_%s_kernel" % name])
        w["head_%s_bias" % name] = bias
    return w


def _others(size, seed):
    return (0.5 + 0.25 * np.random.default_rng(seed).random(size)).astype(np.float32)


def _one_large(distance):
    """per head: small biases, and one class `big` whose logit lies `distance` (nats) above them -> (biases, big classes)"""
    biases, big = [], []
    for k, size in enumerate(HEAD_SIZE):
        bias = _others(size, k)
        b = (5 * k + 2) % size
        bias[b] = np.float32((distance + np.log(size - 1.0)) / R.SELU_SCALE + 0.625)
        biases.append(bias)
        big.append(b)
    return biases, big


def _labels_avoiding(big, rows=8):
    return np.array([[(b + 1 + 3 * r) % size if (b + 1 + 3 * r) % size != b else (b + 2) % size for b, size in zip(big, HEAD_SIZE)] for r in range(rows)], dtype=np.uint8)


def _loss_case(name):
    """-> (head biases, labels [8, 4], what every (row, head) must be: the regime of (p_y, smallest 1 - p of a wrong class))"""
    if name in ("both_clips", "just_unclipped", "true_class_saturated", "ce_floor"):
        distance = {"both_clips": np.log(1 / 7e-10), "just_unclipped": np.log(1 / 5e-5), "true_class_saturated": np.log(1 / 7e-10), "ce_floor": np.log(1e13)}[name]
        biases, big = _one_large(distance)
        labels = _labels_avoiding(big)
        want = np.full((8, 4), {"both_clips": "clipped", "just_unclipped": "unclipped", "true_class_saturated": "clipped", "ce_floor": "floor"}[name], dtype=object)
        if name == "true_class_saturated":           # six rows of each head have the large class as their label; the other two keep the sums away from 0
            for k in range(4):
                for r in range(8):
                    if (r + k) % 4 != 0:
                        labels[r, k] = big[k]
                        want[r, k] = "saturated"
        return biases, labels, want
    biases = [(0.1 + 2.9 * np.random.default_rng(10 + k).random(size)).astype(np.float32) for k, size in enumerate(HEAD_SIZE)]
    labels = np.stack([np.random.default_rng(20 + k).integers(0, size, 8) for k, size in enumerate(HEAD_SIZE)], axis=1).astype(np.uint8)
    return biases, labels, np.full((8, 4), "ordinary", dtype=object)


def _assert_regime(p, labels, want, loss):
    """conditions on the float64 reference, before anything is compared: the clipped quantities lie below 1e-9 or above 1e-6, never between"""
    for r in range(8):
        for k, (off, size) in enumerate(zip(HEAD_OFF, HEAD_SIZE)):
            ph = p[r, off:off + size]
            y = labels[r, k]
            p_y, q_wrong = ph[y], np.delete(1.0 - ph, y).min()
            if loss == "CrossEntropy":
                assert (p_y < 1e-12) == (want[r, k] == "floor") and (p_y < 1e-12 or p_y > 1e-6), (r, k, p_y)
                continue
            assert (p_y < 1e-9 or p_y > 1e-6) and (q_wrong < 1e-9 or q_wrong > 1e-6), (r, k, p_y, q_wrong)
            if want[r, k] == "clipped":
                assert p_y < 1e-9 and q_wrong < 1e-9, (r, k, p_y, q_wrong)
            elif want[r, k] == "unclipped":
                assert 1e-6 < p_y < 1e-4 and 1e-6 < q_wrong < 1e-4, (r, k, p_y, q_wrong)
            elif want[r, k] == "saturated":
                assert 1.0 - p_y < 1e-9 and q_wrong > 1e-6, (r, k, p_y, q_wrong)
            else:
                assert p_y > 1e-6 and q_wrong > 1e-6, (r, k, p_y, q_wrong)


def _check_loss(t, name, loss, class_weights=None):
    biases, labels, want = _loss_case(name)
    x, _ = synth.synthetic_input(8, seed=3)
    t.set_tensors(_loss_weights(biases))
    t.config(class_weights=class_weights, dropout_rates=NO_DROPOUT)
    t.zero_grad()
    losses = t.accumulate(x, labels, training=True)
    probs = t.probabilities()
    grads = t.get_tensors("gradients")
    # the reference: the losses as tools/torch_train_ref.py writes them, float64, from the exact logits
    row = np.concatenate([SELU_SCALE32 * b for b in biases])
    assert row.dtype == np.float32
    logits = torch.tensor(np.tile(row.astype(np.float64), (8, 1)), requires_grad=True)
    parts, p = R.head_losses(logits, labels, loss, class_weights)
    sum(parts).backward()
    p = p.detach().numpy()
    _assert_regime(p, labels, want, loss)
    parts = np.array([v.item() for v in parts])
    dz = logits.grad.numpy() * float(SELU_SCALE32)                  # every pre-activation is positive: selu' = scale
    print("%s %s: losses %s, worst relative error %.3g" % (loss, name, parts, float(np.abs(losses / parts - 1).max())))
    assert np.isfinite(losses).all() and np.isfinite(probs).all() and all(np.isfinite(g).all() for g in grads.values())
    assert (np.abs(losses - parts) <= 1e-9 * np.abs(parts)).all(), (losses, parts)
    ulp = np.spacing(np.abs(p).astype(np.float32)).astype(np.float64)
    assert (np.abs(probs.astype(np.float64) - p) <= 2 * ulp).all(), float((np.abs(probs - p) / ulp).max())
    worst = 0.0
    for (head, off, size) in R.HEADS:
        want_g, bound = dz[:, off:off + size].sum(axis=0), 8 * EPS32 * np.abs(dz[:, off:off + size]).sum(axis=0)
        got = grads["head_%s_bias" % head].astype(np.float64)
        worst = max(worst, float((np.abs(got - want_g) / bound).max()))
        assert (np.abs(got - want_g) <= bound).all(), (head, float((np.abs(got - want_g) / bound).max()))
    print("%s %s: head bias gradients, worst error / bound %.3g" % (loss, name, worst))


@pytest.mark.parametrize("name", ["both_clips", "just_unclipped", "true_class_saturated", "ordinary"])
def test_focal_loss_known_answers(trainer, name):
    """both_clips: p_y < 1e-9 and a wrong class with 1 - p < 1e-9 in every row; just_unclipped: both in (1e-6, 1e-4); true_class_saturated: the label
    itself at 1 - p_y < 1e-9 in six rows of each head (loss and gradient almost 0; nothing may be NaN); ordinary: a control"""
    _check_loss(trainer, name, "FocalLoss")


@pytest.mark.parametrize("name", ["ce_floor", "ordinary"])
def test_cross_entropy_known_answers(name):
    """ce_floor: p_y < 1e-12, the 1e-10 inside the log decides the loss and the gradient; class weights 0.5 .. 2"""
    t = _capi.Trainer(0, 8, "Adam", "CrossEntropy")
    try:
        _check_loss(t, name, "CrossEntropy", np.linspace(0.5, 2.0, 90))
    finally:
        t.close()


# ---- the default micro-batch in place -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_trainer():
    t = _capi.Trainer(0, 1024, "Adam", "FocalLoss")
    t.set_tensors(weights.synthetic_weights())
    yield t
    t.close()


@pytest.fixture(scope="module")
def batch_1024():
    x, _ = synth.synthetic_input(1024, seed=7)
    rng = np.random.default_rng(8)
    return x, np.stack([rng.integers(0, s, 1024) for s in HEAD_SIZE], axis=1).astype(np.uint8)


@pytest.mark.parametrize("rates", [R.DEFAULT_RATES, NO_DROPOUT], ids=["dropout_on", "dropout_off"])
def test_1024_rows_whole_and_in_16_pieces(default_trainer, batch_1024, rates):
    """Fresh weights, 1 024 rows in one micro-batch and as 16 pieces of 64 with first_row set.  A row's forward arithmetic does not depend on the
    row block it lands in: probabilities and masks are the same bits, the loss sums the same row losses in another order.  The gradients are
    measured against the float64 sum of the 16 pieces' own gradients (docs/train.md records the ratios) and only held to be finite: the bounds
    of the summation order are asserted where the host knows the terms, in the rounding tests above."""
    t, (x, lab) = default_trainer, batch_1024
    t.config(dropout_rates=rates, seed=11)
    t.zero_grad()
    losses_whole = t.accumulate(x, lab)
    probs_whole = t.probabilities()
    masks_whole = [t.read_mask(k) for k in range(6)]
    g_whole = t.get_tensors("gradients")
    g_ref = {k: np.zeros(v.shape, dtype=np.float64) for k, v in g_whole.items()}
    losses_pieces = np.zeros(4)
    for first in range(0, 1024, 64):
        t.zero_grad()
        losses_pieces += t.accumulate(x[first:first + 64], lab[first:first + 64], first_row=first)
        assert np.array_equal(t.probabilities().view(np.uint32), probs_whole[first:first + 64].view(np.uint32)), first
        for k in range(6):
            whole = masks_whole[k][:, first:first + 64] if k == 0 else masks_whole[k][first:first + 64]
            assert np.array_equal(t.read_mask(k), whole), (first, k)
        for k, v in t.get_tensors("gradients").items():
            g_ref[k] += v
    assert (np.abs(losses_pieces - losses_whole) <= 1024 * 2.0 ** -53 * np.abs(losses_whole)).all(), (losses_pieces, losses_whole)
    t.zero_grad()
    for first in range(0, 1024, 64):
        t.accumulate(x[first:first + 64], lab[first:first + 64], first_row=first)
    g_acc = t.get_tensors("gradients")
    what = "dropout on" if any(rates) else "dropout off"
    for k in g_ref:
        assert np.isfinite(g_whole[k]).all() and np.isfinite(g_acc[k]).all() and np.abs(g_whole[k]).max() > 0, k
        norm = np.linalg.norm(g_ref[k])
        print("n=1024 %s %-22s ||G_whole - G_ref|| / ||G_ref|| = %.3g   ||G_acc - G_ref|| / ||G_ref|| = %.3g" % (
            what, k, np.linalg.norm(g_whole[k] - g_ref[k]) / norm, np.linalg.norm(g_acc[k] - g_ref[k]) / norm))


# ---- bad arguments launch nothing -----------------------------------------------------------------------------------------------------------
GOOD_GEMM = _laid_out(M=33, N=21, K=17, batch=4, bias=True, accumulate=1)


def _raw_gemm(t, g, a, b, c, bias, counts=None, null=None):
    """clair_train_debug_gemm as C sees it -> (return code, message)"""
    dims = np.array([g[k] for k in ("M", "N", "K", "batch", "accumulate")], dtype=np.int64)
    strides = np.array([g[k] for k in STRIDE_NAMES], dtype=np.int64)
    ptr = {"a": _capi._ptr(a), "b": _capi._ptr(b), "bias": _capi._ptr(bias), "c": _capi._ptr(c), "dims": _capi._ptr(dims), "strides": _capi._ptr(strides)}
    count = dict({"a": a.size, "b": b.size, "bias": bias.size, "c": c.size}, **(counts or {}))
    if null:
        ptr[null] = None
    rc = t._lib.clair_train_debug_gemm(t._h, ptr["a"], count["a"], ptr["b"], count["b"], ptr["bias"], count["bias"], ptr["c"], count["c"], ptr["dims"], ptr["strides"])
    return rc, t._lib.clair_train_last_error(t._h).decode()


def test_debug_gemm_refuses_bad_arguments(trainer):
    rng = np.random.default_rng(1)
    draw = lambda shape: rng.integers(-2, 3, shape).astype(np.float32)      # noqa: E731
    a, b, c0, bias = _operands(GOOD_GEMM, draw, draw, draw, draw, margin=0)
    sizes = dict(zip(("a", "b", "c", "bias"), (_span(*shape) for shape in _shapes(GOOD_GEMM))))
    assert (a.size, b.size, c0.size, bias.size) == (sizes["a"], sizes["b"], sizes["c"], sizes["bias"])
    word = {"a": "A:", "b": "B:", "c": "C:", "bias": "bias:"}
    for operand in ("a", "b", "c", "bias"):                         # one element short of the largest index
        c = c0.copy()
        rc, message = _raw_gemm(trainer, GOOD_GEMM, a, b, c, bias, counts={operand: sizes[operand] - 1})
        assert rc != 0 and word[operand] in message and "largest element index %d" % (sizes[operand] - 1) in message, message
        assert np.array_equal(c, c0)
    for axis, operand in (("M", "A:"), ("N", "B:"), ("K", "A:"), ("batch", "A:")):                  # one more row, column, term or batch than the arrays hold
        rc, message = _raw_gemm(trainer, dict(GOOD_GEMM, **{axis: GOOD_GEMM[axis] + 1}), a, b, c0.copy(), bias)
        assert rc != 0 and operand in message and "largest element index" in message, message
    for name in STRIDE_NAMES:
        rc, message = _raw_gemm(trainer, dict(GOOD_GEMM, **{name: -1}), a, b, c0.copy(), bias)
        assert rc != 0 and "stride %s is -1" % name in message, message
    for axis in ("M", "N", "K", "batch"):
        for value in (0, -3):
            rc, message = _raw_gemm(trainer, dict(GOOD_GEMM, **{axis: value}), a, b, c0.copy(), bias)
            assert rc != 0 and "%s is %d" % (axis, value) in message, message
    rc, message = _raw_gemm(trainer, dict(GOOD_GEMM, accumulate=2), a, b, c0.copy(), bias)
    assert rc != 0 and "accumulate is 2" in message, message
    rc, message = _raw_gemm(trainer, dict(GOOD_GEMM, M=1 << 21), a, b, c0.copy(), bias)
    assert rc != 0 and "M is 2097152" in message, message
    rc, message = _raw_gemm(trainer, dict(GOOD_GEMM, sam=1 << 40), a, b, c0.copy(), bias)
    assert rc != 0 and "stride sam" in message, message
    for null, named in (("a", "A is NULL"), ("b", "B is NULL"), ("c", "C is NULL"), ("bias", "bias is NULL"), ("dims", "dims is NULL"), ("strides", "strides is NULL")):
        rc, message = _raw_gemm(trainer, GOOD_GEMM, a, b, c0.copy(), bias, null=null)
        assert rc != 0 and named in message, message
    assert trainer._lib.clair_train_debug_gemm(None, None, 0, None, 0, None, 0, None, 0, None, None) != 0
    assert b"handle is NULL" in trainer._lib.clair_train_last_error(None)
    with pytest.raises(_capi.EngineError) as ei:
        trainer.debug_gemm(a, b, c0[:-1], (33, 21, 17, 4, 1), [GOOD_GEMM[k] for k in STRIDE_NAMES], bias)
    assert "clair_train_debug_gemm" in str(ei.value) and "C:" in str(ei.value)
    _check_exact(trainer, GOOD_GEMM, seed=2)                        # the handle still works


def _raw_column_sum(t, x, x_count, rows, cols, ld, out, out_count, d=1, s1=1, s2=0):
    rc = t._lib.clair_train_debug_column_sum(t._h, None if x is None else _capi._ptr(x), x_count, rows, cols, ld, None if out is None else _capi._ptr(out), out_count, d, s1, s2)
    return rc, t._lib.clair_train_last_error(t._h).decode()


def test_debug_column_sum_refuses_bad_arguments(trainer):
    rows, cols, ld = 9, 21, 24
    x = np.ones((rows - 1) * ld + cols, dtype=np.float32)
    out0 = np.full(cols, 3.0, dtype=np.float32)
    bad = [
        (dict(x_count=x.size - 1), "x: the largest element index %d" % (x.size - 1)),
        (dict(out_count=cols - 1), "out: the largest element index %d" % (cols - 1)),
        (dict(rows=rows + 1), "x: the largest element index"),
        (dict(cols=cols + 1), "x: the largest element index"),
        (dict(ld=ld + 1), "x: the largest element index"),
        (dict(s1=2), "out: the largest element index %d" % (2 * (cols - 1))),
        (dict(d=4, s1=1, s2=6), "out: the largest element index %d" % (5 + 3 * 6)),
        (dict(ld=-1), "stride ld is -1"), (dict(s1=-1), "stride s1 is -1"), (dict(d=2, s2=-1), "stride s2 is -1"),
        (dict(rows=0), "rows is 0"), (dict(rows=-2), "rows is -2"), (dict(cols=0), "cols is 0"), (dict(cols=-2), "cols is -2"), (dict(d=0), "d is 0"), (dict(d=-1), "d is -1"),
        (dict(x=None), "x is NULL"), (dict(out=None), "out is NULL"),
    ]
    for change, named in bad:
        out = out0.copy()
        args = dict(dict(x=x, x_count=x.size, rows=rows, cols=cols, ld=ld, out=out, out_count=cols, d=1, s1=1, s2=0), **change)
        rc, message = _raw_column_sum(trainer, **args)
        assert rc != 0 and "clair_train_debug_column_sum" in message and named in message, (change, message)
        assert np.array_equal(out, out0)
    assert trainer._lib.clair_train_debug_column_sum(None, None, 0, 1, 1, 1, None, 0, 1, 1, 0) != 0
    assert b"handle is NULL" in trainer._lib.clair_train_last_error(None)
    with pytest.raises(_capi.EngineError):
        trainer.debug_column_sum(x[:-1], rows, cols, ld, out0)
    _column_sum_case(trainer, np.random.default_rng(4), rows, cols, ld)       # the handle still works
