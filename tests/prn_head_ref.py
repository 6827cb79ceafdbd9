"""Reference side of the recorded PRN step's kernels (csrc/losses.hip: mpn_prn_head_train, mpn_dropout_dev, mpn_prn_pack), shared by
tests/test_prn_replay_gpu.py and tests/test_prn_replay_cpu.py.  Test-side only; numpy on the CPU.

The loss head's contract has two halves.  The gradient dl is compared BYTE FOR BYTE with the kernel chain it replaces
(mpn_add_softmax_rows -> mpn_bce_mean_backward -> mpn_softmax_rows_backward -> cast) run on the same operands, pad lanes exactly 0.
The loss is compared with loss_ref.bce_ref's float64 value on the float32 probabilities the chain stored (the head forms the same
ones: same expressions, same reductions) under bce_ref's own bound with the head's summation tree in place of the chunked one:
one lane adds ceil(cols / 256) terms, then the block tree (loss_ref.BLOCK_LEVELS), then double precision over the row partials —
`levels * u * sum |terms|` with levels = ceil(cols / 256) + BLOCK_LEVELS.  Nothing is fitted to the kernel.

`chain_model` / `head_model` are float32 numpy models of the two routes with the kernels' summation order (lane-strided
accumulation, the xor-shuffle wave tree, the four-wave combine in lane 0); the CPU test shows that `check_head` accepts the head
model against the chain model and rejects four modelled faults."""
import numpy as np

import loss_ref as L
from loss_ref import U, f32, f64

HEAD_GS = 1.0          # the recorded step's d(loss)/d(loss)


def head_levels(cols):
    return -(-cols // 256) + L.BLOCK_LEVELS


def head_loss_ref(p, y, cols):
    """(float64 mean BCE, bound) for the head: bce_ref's terms, the head's summation tree.  p, y: [rows, cols] float32."""
    ref, _ = L.bce_ref(p.reshape(-1), y.reshape(-1))
    p64, y64 = p.astype(f64), y.astype(f64)
    n = p64.size
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p64), -100.0), np.maximum(np.log(1 - p64), -100.0)
    with np.errstate(invalid="ignore"):
        t1, t2 = np.where(y64 == 0, 0.0, y64 * lp), np.where(y64 == 1, 0.0, (1 - y64) * lq)
    term = -(t1 + t2)
    qa = np.where((p64 < 0.5) & (lq > -100), 2.0 ** -25 / np.maximum(1 - p64, 1e-300), 0.0)
    per = (L.R_LOG + 3) * U * (np.abs(t1) + np.abs(t2)) + np.abs(1 - y64) * qa
    bound = (per.sum() + head_levels(cols) * U * np.abs(term).sum()) / n + U * abs(ref)
    return ref, bound


def saturating_case(rows=3, cols=8568, seed=5):
    """3 x 8568 (prn_coeff 1: 8 pad lanes), about 1 % ones; a few dominant entries per row push their p towards 1 (p (1 - p) under
    the 1e-12 clamp, or 1 - p == 0) and everything else towards 0 (some underflow to exactly 0), and every 7th pre-activation is
    exactly 0 (masked: the ReLU test is a strict >)."""
    r = L.rng(seed)
    stride = L.round_up(cols, 32)
    o = np.full((rows, stride), 777.0, f32)
    o[:, :cols] = r.standard_normal((rows, cols)).astype(f32) * 2
    o[:, 0:cols:7] = 0.0
    res = r.standard_normal((rows, cols)).astype(f32)
    o[0, 11] = 60.0                                   # row 0: one entry takes all the mass: p == 1 there, the rest ~ e^-60
    o[1, 100] = 40.0
    o[1, 200] = 40.0                                  # row 1: two entries share it, the rest ~ e^-40
    o[2, 5] = 120.0                                   # row 2: the rest underflow to exactly 0
    y = (r.random_sample((rows, cols)) < 0.01).astype(f32)
    y[0, 11], y[1, 100], y[1, 200], y[2, 5] = 1.0, 0.0, 1.0, 1.0
    return dict(cols=cols, stride=stride, a=o, res=res, y=y)


def softmax_label(c, seed=1):
    """Labels for a loss_ref.softmax_case: about half ones, a few soft values."""
    r = L.rng(seed + c["cols"])
    y = (r.random_sample((L.SM_ROWS, c["cols"])) < 0.5).astype(f32)
    y[:, 0:c["cols"]:11] = r.random_sample(y[:, 0:c["cols"]:11].shape).astype(f32)
    return y


# ------------------------------------------------------------------------------------------------ float32 models
def _wave_tree(v, op):
    """v: [64] float32 -> what every lane holds after `for m in 32, 16, .., 1: v = op(v, shfl_xor(v, m))` (lane 0 is read)."""
    v = v.copy()
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = op(v, v[idx ^ m]).astype(f32)
    return v[0]


def _block_reduce(lane_vals, op):
    """lane_vals: [256] float32 per-lane partials -> the block's value (lane 0 combines the four waves left to right)."""
    w = [_wave_tree(lane_vals[k * 64:(k + 1) * 64], op) for k in range(4)]
    if op is np.maximum:
        return np.maximum(np.maximum(w[0], w[1]), np.maximum(w[2], w[3]))
    return f32(f32(f32(w[0] + w[1]) + w[2]) + w[3])


def _lane_sum(terms, fma_with=None):
    """Per-lane strided accumulation s += terms[i] (i = lane, lane + 256, ..); with `fma_with` the step is fma(terms, fma_with, s)."""
    cols = terms.shape[0]
    s = np.zeros(256, f32)
    for base in range(0, cols, 256):
        t = terms[base:base + 256]
        k = t.shape[0]
        if fma_with is None:
            s[:k] = (s[:k] + t).astype(f32)
        else:
            s[:k] = (t.astype(f64) * fma_with[base:base + 256].astype(f64) + s[:k].astype(f64)).astype(f32)
    return s


def _lane_max(vals):
    cols = vals.shape[0]
    m = np.full(256, -np.inf, f32)
    for base in range(0, cols, 256):
        t = vals[base:base + 256]
        m[:t.shape[0]] = np.maximum(m[:t.shape[0]], t)
    return m


def _row_prob(a_row, res_row):
    t = (np.maximum(a_row, f32(0)) + res_row).astype(f32)
    mx = _block_reduce(_lane_max(t), np.maximum)
    with np.errstate(under="ignore"):
        e = np.exp((t - mx).astype(f32)).astype(f32)
    s = _block_reduce(_lane_sum(e), np.add)
    inv = f32(1) / f32(s)
    return (e * inv).astype(f32)


def _dprob(p, y, gs, n):
    k = f32(f32(gs) / f32(n))
    return (k * (p - y).astype(f32) / np.maximum((p * (f32(1) - p).astype(f32)).astype(f32), f32(1e-12))).astype(f32)


def _row_loss_terms(p, y):
    with np.errstate(divide="ignore"):
        lp = np.maximum(np.log(p).astype(f32), f32(-100))
        lq = np.maximum(np.log((f32(1) - p).astype(f32)).astype(f32), f32(-100))
    return (-((y * lp).astype(f32) + ((f32(1) - y).astype(f32) * lq).astype(f32)).astype(f32)).astype(f32)


def chain_model(a, res, y, cols, npad, gs=HEAD_GS):
    """The four-kernel route: p stored, dp stored over the flat [rows * cols] array, softmax backward per row, cast / pad copy.
    Returns (dl [rows, npad] float32 — the values before the storage cast —, p [rows, cols])."""
    rows = a.shape[0]
    p = np.stack([_row_prob(a[r, :cols], res[r]) for r in range(rows)])
    dp = _dprob(p, y, gs, rows * cols)
    dl = np.zeros((rows, npad), f32)
    for r in range(rows):
        dot = _block_reduce(_lane_sum(p[r], fma_with=dp[r]), np.add)
        g = (p[r] * (dp[r] - dot).astype(f32)).astype(f32)
        dl[r, :cols] = np.where(a[r, :cols] > 0, g, f32(0))
    return dl, p


def head_model(a, res, y, cols, npad, gs=HEAD_GS, mut=None):
    """The one-launch route: everything per row, p and dp recomputed per pass, one loss partial per row, double finalize.
    Returns (dl [rows, npad] float32, loss float32).  `mut`: one of the modelled faults."""
    rows = a.shape[0]
    n = rows * cols
    dl = np.zeros((rows, npad), f32)
    part = np.zeros(rows, f32)
    dots = []
    for r in range(rows):
        p = _row_prob(a[r, :cols], res[r])
        dp = _dprob(p, y[r], gs, 1 if mut == "1/N omitted" else n)
        dots.append(_block_reduce(_lane_sum(p, fma_with=dp), np.add))
        part[r] = _block_reduce(_lane_sum(_row_loss_terms(p, y[r])), np.add)
    for r in range(rows):
        p = _row_prob(a[r, :cols], res[r])
        dp = _dprob(p, y[r], gs, 1 if mut == "1/N omitted" else n)
        dot = dots[(r + 1) % rows] if mut == "dot product of the neighbouring row" else dots[r]
        g = (p * (dp - dot).astype(f32)).astype(f32)
        dl[r, :cols] = g if mut == "ReLU mask dropped" else np.where(a[r, :cols] > 0, g, f32(0))
    if mut == "non-zero pad lane" and npad > cols:
        dl[rows - 1, npad - 1] = f32(2.0 ** -20)
    loss = f32(part.astype(f64).sum() / n)
    return dl, loss


# ------------------------------------------------------------------------------------------------ the check both tests use
def check_head(tag, dl_bytes, loss, chain_dl_bytes, p_chain, y, cols, npad):
    """dl_bytes / chain_dl_bytes: uint8 views [rows, npad * itemsize] of the head's gradient and of the chain's (already cast and
    padded); p_chain: the float32 probabilities the chain stored.  Asserts byte equality, zero pad lanes and the loss bound;
    returns (loss error, bound)."""
    dl_bytes, chain_dl_bytes = np.asarray(dl_bytes), np.asarray(chain_dl_bytes)
    assert dl_bytes.shape == chain_dl_bytes.shape, tag
    item = dl_bytes.shape[1] // npad
    pad = dl_bytes[:, cols * item:]
    assert not pad.any(), "%s: %d non-zero bytes in the pad lanes" % (tag, int(np.count_nonzero(pad)))
    diff = np.nonzero(dl_bytes != chain_dl_bytes)
    assert diff[0].size == 0, "%s: dl differs from the chain's in %d bytes, first at row %d column %d" % (
        tag, diff[0].size, diff[0][0], diff[1][0] // item)
    ref, bound = head_loss_ref(p_chain, y, cols)
    err = abs(float(loss) - ref)
    L.report("%-60s loss err=%.3e  bound=%.3e  ref=%.6e  %s" % (tag, err, bound, ref, "OK" if err <= bound else "FAIL"))
    assert np.isfinite(float(loss)) and err <= bound, "%s: loss %.9e vs %.9e: err %.3e > bound %.3e" % (tag, float(loss), ref, err, bound)
    return err, bound
