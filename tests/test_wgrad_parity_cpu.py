"""Teeth for the weight-gradient parity bound (CPU tier).

tests/test_wgrad_parity_gpu.py compares every element of dw = dw0 + sum_p dy[p] x_tap[p] (and of the fused bias gradient
db = db0 + sum_p dy[p]) with a float64 reference under helpers.check_elementwise, with K = the pixels of one split-K slice and
extra_terms = slices + 1 (the ordered reduction of the slice partials and the add into the prefilled dw).  Here the kernels'
arithmetic is modelled in fp32 blocked form — k-steps of 32 pixels (16-bit MFMA) or 4 (exact-fp32 MFMA), each step's sum rounded
to fp32 and accumulated per slice, then the slices added into dw0 in order — at the slice structures the GPU cases run:

  * the bound accepts the exact result and blocked sums in other step and slice orders;
  * it rejects a dropped k-step in an interior slice, a slice partial missing or counted twice, a 3x3 tap shifted by one pixel at
    the halo, a pixel attributed to the neighbouring pyramid level at a seg_chunk0 boundary, a virtual-concatenation member read
    with the wrong up-sampling shift, dw overwritten instead of accumulated, and a bias gradient missing one slice.

Operands are scaled like the GPU cases (unit normals), so one k-step (~sqrt(32) in magnitude) is orders of magnitude above the
bound (~0.05 at 16 400 pixels)."""
import pytest
import torch
import torch.nn.functional as F

from helpers import check_elementwise, rng_normal

F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def _cols(x, k, pad):
    """[B, C, H, W] float64 -> the gathered operand [P, C*k*k] (pixel order b, h, w; column order c, r, s) of a stride-1 conv."""
    B, C = x.shape[:2]
    return F.unfold(x, k, padding=pad).transpose(1, 2).reshape(-1, C * k * k)


def _pix(t):
    """[B, O, H, W] -> [P, O]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _slices(P, cp, n):
    return [(min(i * cp, P), min((i + 1) * cp, P)) for i in range(n)]


def _operands(seed, dtype, B, C, H, W, O):
    x = rng_normal(seed, B, C, H, W).to(dtype).double()
    dy = rng_normal(seed + 1, B, O, H, W).to(dtype).double()
    return x, dy


def _blocked(cols, dy, ranges, k_step, dw0, db0, step_order=1, slice_order=None, skip_step=None, skip_slice=None, dup_slice=None,
             skip_bias_slice=None):
    """fp32 model of the kernel: per slice, k-steps of k_step pixels (each step's exact sum rounded to fp32) accumulated in fp32 in
    `step_order` (1 forward, -1 reversed); then dw0 (+)= the slice partials in `slice_order`.  Returns (dw [O, K], db [O]) as float64.
    The bias is the same contraction against a column of ones."""
    a = torch.cat([cols, torch.ones(cols.shape[0], 1, dtype=cols.dtype)], 1)
    parts = []
    for si, (s0, s1) in enumerate(ranges):
        acc = torch.zeros(dy.shape[1], a.shape[1], dtype=F32)
        steps = list(range(s0, s1, k_step))[::step_order]
        for j, p0 in enumerate(steps):
            if skip_step == (si, j):
                continue
            p1 = min(p0 + k_step, s1)
            acc = acc + (dy[p0:p1].t() @ a[p0:p1]).float()
        parts.append(acc)
    out = torch.cat([dw0, db0[:, None]], 1).float()
    order = list(range(len(parts))) if slice_order is None else slice_order
    for si in order:
        if si == skip_slice:
            continue
        p = parts[si]
        if si == skip_bias_slice:
            p = p.clone()
            p[:, -1] = 0
        out = out + p
        if si == dup_slice:
            out = out + p
    return out[:, :-1].double(), out[:, -1].double()


def _ref(cols, dy, dw0, db0):
    """float64 reference and magnitude (|dw0| + sum |dy| |x|) of dw and db."""
    return (dw0 + dy.t() @ cols, db0 + dy.sum(0), dw0.abs() + dy.abs().t() @ cols.abs(), db0.abs() + dy.abs().sum(0))


def _checker(tag, ref, k_step, cp, n_slices):
    dw_ref, db_ref, dw_mag, db_mag = ref

    def check(what, got):
        dw, db = got
        check_elementwise("cpu wgrad teeth %s %s dw" % (tag, what), dw, dw_ref, dw_mag, F32, k_step, cp, n_slices + 1, names="oi")
        check_elementwise("cpu wgrad teeth %s %s db" % (tag, what), db, db_ref, db_mag, F32, k_step, cp, n_slices + 1, names="o")
    return check


def _rejects(check, what, got):
    with pytest.raises(AssertionError):
        check("REJECT " + what, got)


def _prefill(seed, O, K):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(O, K, generator=g, dtype=torch.float64).float().double(), torch.randn(O, generator=g, dtype=torch.float64).float().double()


# 3x3 over B=4, 50 x 82 (16 400 pixels) in 32 slices of 544 pixels, slice 31 empty: the slice structure mpn_conv_wgrad_chunks gives the
# 1x1 256->1024 GPU case at that pixel count (fewer channels here: the bound is per element and does not depend on them)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_wgrad_bound_single_tensor(dtype):
    B, C, H, W, O, cp, n = 4, 16, 50, 82, 8, 544, 32
    k_step = 32 if dtype != F32 else 4
    x, dyt = _operands(11, dtype, B, C, H, W, O)
    cols, dy = _cols(x, 3, 1), _pix(dyt)
    P = cols.shape[0]
    ranges = _slices(P, cp, n)
    assert ranges[-1][0] == ranges[-1][1] == P and ranges[-2][1] - ranges[-2][0] == 80     # last slice empty, the one before short
    dw0, db0 = _prefill(12, O, cols.shape[1])
    ref = _ref(cols, dy, dw0, db0)
    check = _checker(str(dtype), ref, k_step, cp, n)
    tag = str(dtype)

    # correct results pass: the exact result, and fp32 blocked sums in forward / reversed step order and permuted slice order
    check("exact", (ref[0].float().double(), ref[1].float().double()))
    check("blocked", _blocked(cols, dy, ranges, k_step, dw0, db0))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).tolist()
    good = _blocked(cols, dy, ranges, k_step, dw0, db0, step_order=-1, slice_order=perm)
    check("blocked reversed steps, permuted slices", good)

    # bugs fail
    _rejects(check, "k-step dropped in slice 13", _blocked(cols, dy, ranges, k_step, dw0, db0, skip_step=(13, 5)))
    _rejects(check, "slice 7 missing", _blocked(cols, dy, ranges, k_step, dw0, db0, skip_slice=7))
    _rejects(check, "slice 7 twice", _blocked(cols, dy, ranges, k_step, dw0, db0, dup_slice=7))
    _rejects(check, "dw overwritten", _blocked(cols, dy, ranges, k_step, torch.zeros_like(dw0), db0))          # dw overwritten, not accumulated
    got = _blocked(cols, dy, ranges, k_step, dw0, db0, skip_bias_slice=20)
    check_elementwise("cpu wgrad teeth %s bias slice missing: dw intact" % tag, got[0], ref[0], ref[2], F32, k_step, cp, n + 1, names="oi")
    with pytest.raises(AssertionError):
        check_elementwise("cpu wgrad teeth %s bias slice missing" % tag, got[1], ref[1], ref[3], F32, k_step, cp, n + 1, names="o")
    # tap (r, 0) of the left border column reads image column 0 instead of the zero halo (a one-pixel shift of the halo predicate)
    c6 = cols.clone().view(B, H, W, C, 3, 3)
    xp = F.pad(x, (1, 1, 1, 1))
    for r in range(3):
        c6[:, :, 0, :, r, 0] = xp[:, :, r:r + H, 1].permute(0, 2, 1)
    _rejects(check, "halo tap shifted", _blocked(c6.view(P, -1), dy, ranges, k_step, dw0, db0))


# pyramid: five levels shaped like p3..p7 (B=2: 60, 30, 15, 8, 4; levels of 128 and 32 pixels), 3x3, the slice length 512 that
# mpn_conv_wgrad_seg_plan gives the 256->9 head there: 15 + 4 + 1 + 1 + 1 = 22 slices
def test_wgrad_bound_pyramid_level_boundary():
    B, C, O, cp = 2, 16, 8, 512
    levels = (60, 30, 15, 8, 4)
    xs, dys = [], []
    for i, s in enumerate(levels):
        x, dy = _operands(20 + 2 * i, torch.bfloat16, B, C, s, s, O)
        xs.append(_cols(x, 3, 1))
        dys.append(_pix(dy))
    ranges, off, chunk0 = [], 0, [0]
    for c in xs:
        P = c.shape[0]
        nl = (P + cp - 1) // cp
        ranges += [(off + a, off + b) for a, b in _slices(P, cp, nl)]
        off += P
        chunk0.append(len(ranges))
    assert chunk0 == [0, 15, 19, 20, 21, 22]
    cols, dy = torch.cat(xs), torch.cat(dys)
    dw0, db0 = _prefill(30, O, cols.shape[1])
    ref = _ref(cols, dy, dw0, db0)
    check = _checker("pyramid", ref, 32, cp, len(ranges))
    check("blocked", _blocked(cols, dy, ranges, 32, dw0, db0))
    check("blocked reversed", _blocked(cols, dy, ranges, 32, dw0, db0, step_order=-1, slice_order=list(range(len(ranges)))[::-1]))
    # the first pixel of slice seg_chunk0[1] (level p4) gathered from level p3's tensors (a level lookup one slice late)
    P0 = xs[0].shape[0]
    cm, dm = cols.clone(), dy.clone()
    cm[P0], dm[P0] = xs[0][0], dys[0][0]
    _rejects(check, "p4 pixel from p3", _blocked(cm, dm, ranges, 32, dw0, db0))
    # the same at the boundary into the 4 x 4 level (slice seg_chunk0[4], the level's only slice)
    P3 = sum(c.shape[0] for c in xs[:4])
    cm, dm = cols.clone(), dy.clone()
    cm[P3], dm[P3] = xs[3][0], dys[3][0]
    _rejects(check, "p7 pixel from p6", _blocked(cm, dm, ranges, 32, dw0, db0))
    _rejects(check, "k-step dropped in p4 tail slice", _blocked(cols, dy, ranges, 32, dw0, db0, skip_step=(chunk0[2] - 1, 0)))   # p4's last (short) slice


# virtual concatenation [q3, q2] (engine: the keypoint head's conv2): members of 4 channels up-sampled by 2 and 1 (shifts 1, 0) to
# B=2, 64 x 64, read at (h >> shift, w >> shift); 16 slices of 512 pixels (mpn_conv_wgrad_chunks for 3x3 256->19 there)
def test_wgrad_bound_virtual_concat_shift():
    B, H, W, O, cp, n = 2, 64, 64, 8, 512, 16
    mem = [rng_normal(40 + s, B, 4, H >> s, W >> s).to(torch.bfloat16).double() for s in (1, 0)]

    def cat(shifts):
        return torch.cat([m[:, :, torch.arange(H) >> s][:, :, :, torch.arange(W) >> s] for m, s in zip(mem, shifts)], 1)
    cols = _cols(cat((1, 0)), 3, 1)
    dy = _pix(rng_normal(43, B, O, H, W).to(torch.bfloat16).double())
    ranges = _slices(cols.shape[0], cp, n)
    dw0, db0 = _prefill(44, O, cols.shape[1])
    ref = _ref(cols, dy, dw0, db0)
    check = _checker("kseg", ref, 32, cp, n)
    check("blocked", _blocked(cols, dy, ranges, 32, dw0, db0, step_order=-1))
    _rejects(check, "q3 shift 2", _blocked(_cols(cat((2, 0)), 3, 1), dy, ranges, 32, dw0, db0))       # q3 read at shift 2 instead of 1
    _rejects(check, "q2 shift 1", _blocked(_cols(cat((1, 1)), 3, 1), dy, ranges, 32, dw0, db0))       # q2 read as if up-sampled


def test_wgrad_bound_margin_of_one_kstep():
    """The GPU shapes are chosen so that one k-step is far above the bound: at 16 400 pixels in 32 slices of 544 the bound of a
    typical element is ~0.05, a k-step of unit normals ~sqrt(32) = 5.7; and a dropped k-step breaks the bound in nearly every
    element, not only in a lucky few."""
    from helpers import U24
    K, slices, k_step, P = 544, 32, 32, 16400
    mag = P * (2 / torch.pi)                       # E|dy||x| = 2/pi for unit normals
    bound = (K / k_step + k_step + slices + 1 + 2) * U24 * mag
    assert bound < 0.06 and 32 ** 0.5 / bound > 100
    g = torch.Generator().manual_seed(5)
    step = (torch.randn(32, 4096, generator=g, dtype=torch.float64) * torch.randn(32, 4096, generator=g, dtype=torch.float64)).sum(0)
    assert float((step.abs() > bound).double().mean()) > 0.98
