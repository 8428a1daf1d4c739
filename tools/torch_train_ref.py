"""Training oracle on torch-CPU autograd (dev-time checker only, like tools/torch_ref.py; never imported by the product).

The network of clair/model.py written with explicit LSTM steps on the TF-layout kernels ([in+H, 4H], gate columns i|c~|f|o, no forget
bias), the dropout masks handed in from outside, both losses (model.py:247-263 weighted cross entropy, :784-805 focal loss) and the
lambda * L2 term (:689-709).  loss_and_gradients returns the loss parts and the 22 gradients in float32 or float64.  The TensorFlow-1.x
Adam and Momentum updates and clip_by_global_norm are restated in NumPy float32 (adam_step, momentum_step, clip_by_global_norm).
pre_activations returns the input of every SELU, and clear_of_the_selu_kink moves biases until none of them is near zero for a given
batch, so that the float32 gradients are a fair yardstick for the float64 ones (docs/train.md, "The SELU kink").
"""
from collections import OrderedDict

import numpy as np
import torch

H = 128
HEADS = (("gt21", 0, 21), ("genotype", 21, 3), ("len1", 24, 33), ("len2", 57, 33))
SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946
DROPOUT_SELU_ALPHA = -1.7580993408473766       # clair/selu.py:39
DEFAULT_RATES = (0.5, 0.5, 0.2, 0.2, 0.2, 0.2)  # LSTM2, L4, L5_1..4 (clair/model.py:83-97)


def selu(x):
    """clair/selu.py:26-30"""
    return SELU_SCALE * torch.where(x >= 0.0, x, SELU_ALPHA * torch.nn.functional.elu(x))


def dropout_selu_constants(rate):
    """clair/selu.py:64-66 with fixedPointMean 0, fixedPointVar 1 -> (alpha', a, b)"""
    keep = 1.0 - rate
    alpha = DROPOUT_SELU_ALPHA
    a = np.sqrt(1.0 / (keep * ((1.0 - keep) * alpha ** 2 + 1.0)))
    b = 0.0 - a * (keep * 0.0 + (1.0 - keep) * alpha)
    return alpha, a, b


def dropout_selu(x, mask, rate):
    alpha, a, b = dropout_selu_constants(rate)
    return a * (x * mask + alpha * (1.0 - mask)) + b


def _lstm_direction(X, K, b, reverse):
    """X [T,n,in] -> [T,n,H]; CudnnCompatibleLSTMCell: z = [x, h] K + b, c = sigmoid(f) c + sigmoid(i) tanh(c~), h = sigmoid(o) tanh(c)"""
    T, n = X.shape[0], X.shape[1]
    h = torch.zeros(n, H, dtype=X.dtype)
    c = torch.zeros(n, H, dtype=X.dtype)
    outs = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        z = torch.cat([X[t], h], dim=1) @ K + b
        i, g, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs[t] = h
    return torch.stack(outs)


def _bilstm(X, w, layer):
    fw = _lstm_direction(X, w["lstm%d_fw_kernel" % layer], w["lstm%d_fw_bias" % layer], False)
    bw = _lstm_direction(X, w["lstm%d_bw_kernel" % layer], w["lstm%d_bw_bias" % layer], True)
    return torch.cat([fw, bw], dim=2)


def _network(w, x, masks, rates):
    """-> (SELU'd logits [n,90], the input of every SELU: l3 [n,30,256], l4 [n,192], l5_0..3 [n,96], head_<name> [n,size])"""
    n = x.shape[0]
    z = OrderedDict()
    s = x.reshape(n, 33, 32).transpose(0, 1)
    a1 = _bilstm(s, w, 1)
    a2 = _bilstm(a1, w, 2)
    if masks is not None and rates[0] > 0:
        a2 = a2 * torch.as_tensor(np.asarray(masks[0]), dtype=x.dtype) / (1.0 - rates[0])     # tf.layers.dropout
    z["l3"] = torch.einsum("tnc,ctu->nuc", a2, w["l3_kernel"]) + w["l3_bias"].t().unsqueeze(0)
    z["l4"] = selu(z["l3"]).reshape(n, 7680) @ w["l4_kernel"] + w["l4_bias"]
    l4 = selu(z["l4"])
    if masks is not None:
        l4 = dropout_selu(l4, torch.as_tensor(np.asarray(masks[1]), dtype=x.dtype), rates[1])
    logits = []
    for k, (name, _, _) in enumerate(HEADS):
        z["l5_%d" % k] = l4 @ w["l5_kernel"][k] + w["l5_bias"][k]
        l5 = selu(z["l5_%d" % k])
        if masks is not None:
            l5 = dropout_selu(l5, torch.as_tensor(np.asarray(masks[2 + k]), dtype=x.dtype), rates[2 + k])
        z["head_%s" % name] = l5 @ w["head_%s_kernel" % name] + w["head_%s_bias" % name]
        logits.append(selu(z["head_%s" % name]))
    return torch.cat(logits, dim=1), z


def network(w, x, masks=None, rates=DEFAULT_RATES):
    """w: dict of torch tensors; x [n,33,8,4] torch; masks None (no dropout) or {0: [33,n,256], 1: [n,192], 2..5: [n,96]} of 0/1.
    -> SELU'd logits [n,90]"""
    return _network(w, x, masks, rates)[0]


def pre_activations(w, x, masks=None, rates=DEFAULT_RATES, dtype=torch.float64):
    """the input of every SELU of network(), as arrays in dtype: l3 [n,30,256], l4 [n,192], l5_0..3 [n,96] and the four heads' logits
    before their SELU (head_gt21 [n,21], head_genotype [n,3], head_len1, head_len2 [n,33])"""
    torch.set_num_threads(4)
    with torch.no_grad():
        wt = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in w.items()}
        z = _network(wt, torch.tensor(np.asarray(x), dtype=dtype), masks, rates)[1]
    return OrderedDict((k, v.numpy()) for k, v in z.items())


def sign_disagreements(z32, z64):
    """how many SELU inputs lie on different sides of zero in the two sets of pre_activations"""
    return int(sum(np.count_nonzero((z32[k] >= 0) != (z64[k] >= 0)) for k in z64))


def smallest_pre_activation(z):
    return float(min(np.abs(v).min() for v in z.values()))


def _bias_of(w, key):
    """the bias tensor behind the pre-activations `key`, viewed so that its axes are the pre-activations' without the row axis"""
    if key == "l3":
        return w["l3_bias"].T                   # [c,u] -> [u,c]: a view, written through
    if key.startswith("l5_"):
        return w["l5_bias"][int(key[3:])]
    return w[key + "_bias"]


def clear_of_the_selu_kink(w, x, masks=None, rates=DEFAULT_RATES, factor=64, max_rounds=40):
    """SELU's derivative jumps from scale to scale * alpha at zero, so one unit whose input the float32 and the float64 pass put on
    different sides of zero moves whole gradient tensors by 1e-4 .. 1e-3 of their norm: the float32 oracle stops being a yardstick, and
    a device that differs from both by rounding alone may flip a unit of its own.  -> (a copy of w in which only biases have moved,
    until every SELU input of this batch is at least `margin` from zero, report)

    margin = factor * max |z_f32 - z_f64| over all SELU inputs of this batch under w.  Each round adds 4 * margin to the bias of every
    unit with |z_f64| < margin (a bias serves all rows, and an earlier layer's bias moves the later layers: hence rounds) and
    recomputes.  report: margin, rounds, moved (bias elements that differ from w's), smallest (min |z_f64| afterwards)."""
    w = OrderedDict((k, np.array(v, dtype=np.float32, copy=True)) for k, v in w.items())
    before = {k: v.copy() for k, v in w.items() if k.endswith("_bias")}
    z64 = pre_activations(w, x, masks, rates, torch.float64)
    z32 = pre_activations(w, x, masks, rates, torch.float32)
    margin = factor * max(float(np.abs(z32[k].astype(np.float64) - z64[k]).max()) for k in z64)
    rounds = 0
    while smallest_pre_activation(z64) < margin:
        if rounds == max_rounds:
            raise RuntimeError("clear_of_the_selu_kink: SELU inputs within %.3g of zero after %d rounds" % (margin, rounds))
        rounds += 1
        for k, z in z64.items():
            near = (np.abs(z) < margin).any(axis=0)
            if near.any():
                _bias_of(w, k)[near] += np.float32(4 * margin)
        z64 = pre_activations(w, x, masks, rates, torch.float64)
    moved = int(sum(np.count_nonzero(w[k] != v) for k, v in before.items()))
    return w, dict(margin=margin, rounds=rounds, moved=moved, smallest=smallest_pre_activation(z64))


def head_losses(logits, labels, loss="FocalLoss", class_weights=None):
    """-> ([4 losses summed over the rows], probabilities [n,90])"""
    n = logits.shape[0]
    cw = torch.ones(90, dtype=logits.dtype) if class_weights is None else torch.as_tensor(np.asarray(class_weights), dtype=logits.dtype)
    parts, probs = [], []
    for k, (_, off, size) in enumerate(HEADS):
        p = torch.softmax(logits[:, off:off + size], dim=1)
        y = torch.zeros(n, size, dtype=logits.dtype)
        y[torch.arange(n), torch.as_tensor(np.asarray(labels)[:, k].astype(np.int64))] = 1.0
        if loss == "CrossEntropy":
            parts.append(-torch.sum(y * torch.log(p + 1e-10) * cw[off:off + size]))
        else:
            zeros = torch.zeros_like(p)
            pos = torch.where(y > zeros, y - p, zeros)
            neg = torch.where(y > zeros, zeros, p)
            parts.append(-torch.sum(pos ** 2 * torch.log(torch.clamp(p, 1e-8, 1.0)) + neg ** 2 * torch.log(torch.clamp(1.0 - p, 1e-8, 1.0))))
        probs.append(p)
    return parts, torch.cat(probs, dim=1)


def loss_and_gradients(w, x, labels, loss="FocalLoss", masks=None, rates=DEFAULT_RATES, task_loss_weights=(1, 1, 1, 1, 1), class_weights=None,
                       l2_lambda=0.0, dtype=torch.float64):
    """-> dict(parts float64 [4], l2 (without lambda), total, probabilities [n,90], gradients {key: array in dtype})"""
    torch.set_num_threads(4)
    wt = OrderedDict((k, torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True)) for k, v in w.items())
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    logits = network(wt, xt, masks, rates)
    parts, probs = head_losses(logits, labels, loss, class_weights)
    l2 = sum(torch.sum(v ** 2) / 2 for k, v in wt.items() if not k.endswith("_bias"))
    tw = [float(v) for v in task_loss_weights]
    total = sum(tw[k] * parts[k] for k in range(4)) + tw[4] * l2 * l2_lambda
    total.backward()
    return dict(parts=np.array([p.item() for p in parts]), l2=l2.item(), total=total.item(), probabilities=probs.detach().numpy(),
                gradients=OrderedDict((k, v.grad.numpy()) for k, v in wt.items()))


# ---- the optimizer, TensorFlow 1.x, in NumPy float32 -------------------------------------------------------------------------------------
def global_norm(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads.values())))


def clip_by_global_norm(grads, clip_norm=5.0, dtype=np.float32):
    """tf.clip_by_global_norm: g * clip_norm / max(norm, clip_norm) -> (clipped, norm)"""
    norm = global_norm(grads)
    scale = dtype(clip_norm / max(norm, clip_norm))
    return OrderedDict((k, np.asarray(g, dtype=dtype) * scale) for k, g in grads.items()), norm


def adam_step(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, dtype=np.float32):
    """tf.train.AdamOptimizer (ApplyAdam) at step t = 1, 2, ...: the beta powers are products in the variables' type, as TensorFlow's are."""
    f = dtype
    b1p, b2p = f(1), f(1)
    for _ in range(t):
        b1p, b2p = b1p * f(beta1), b2p * f(beta2)
    lr_t = f(lr) * np.sqrt(f(1) - b2p) / (f(1) - b1p)
    w, g, m, v = (np.asarray(a, dtype=f) for a in (w, g, m, v))
    m = m + (g - m) * (f(1) - f(beta1))
    v = v + (g * g - v) * (f(1) - f(beta2))
    return w - (m * lr_t) / (np.sqrt(v) + f(epsilon)), m, v


def momentum_step(w, g, acc, lr, momentum=0.9, dtype=np.float32):
    """tf.train.MomentumOptimizer without Nesterov"""
    f = dtype
    w, g, acc = (np.asarray(a, dtype=f) for a in (w, g, acc))
    acc = acc * f(momentum) + g
    return w - f(lr) * acc, acc


def regularized(grads, w, coefficient, dtype=np.float32):
    """g + coefficient * w on the kernels (coefficient = task_loss_weights[4] * lambda)"""
    f = dtype
    return OrderedDict((k, np.asarray(g, dtype=f) + (f(coefficient) * np.asarray(w[k], dtype=f) if not k.endswith("_bias") else f(0))) for k, g in grads.items())
