"""Split-exact fp64 references of the f16-split convolution kernels, shared by the GPU route tables (test_gpu_conv_f16s_routes.py,
test_gpu_wino_stream_routes.py, test_gpu_conv3d_routes.py, test_gpu_conv3d_pw_routes.py) and checked on the CPU by test_split_exact_reference.py.  A plain helper module: no tests live here.

Direct form (conv_f16s.hip, conv_stream.hip): split_reference, derived in test_gpu_conv_f16s_routes.py; split_reference_3d is the same for
the 5-D operands of conv3d_f16s.hip and conv3d_pw_f16s.hip.
Row-Winograd form (conv_wino.hip): wino_split_reference, derived in test_gpu_wino_stream_routes.py."""
import torch
import torch.nn.functional as F

SPLIT_BAR = 2.0 ** -18
ACTS = ("gelu", "relu", "lrelu", "tanh", "sigmoid")
TORCH_ACT = {"gelu": F.gelu, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, 0.01), "tanh": torch.tanh, "sigmoid": torch.sigmoid}
WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))      # G of F(2,3): U = G g along kx


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def samples_of(B, nimg):
    s = {0, B - 1}
    if 1 < nimg < B:
        s |= {nimg - 1, nimg}
    return sorted(s)


def device_input(x, dev, view):
    """x on the device; view=True: a contiguous view one float into a buffer fenced by NaNs (a read outside x poisons the output)"""
    if not view:
        return x.to(dev)
    buf = torch.full((x.numel() + 8,), float("nan"), device=dev)
    buf[1:1 + x.numel()] = x.reshape(-1).to(dev)
    xd = buf[1:1 + x.numel()].view(x.shape)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    return xd


def split_x(x):
    xh = x.half()
    return xh.double(), (x - xh.float()).half().double()


def split_w(w, s):
    ws = w.float() * (2.0 ** s)
    wh = ws.half()
    return wh.double(), (ws - wh.float()).half().double()


def split_reference(x, w, b, s, conv):
    """fp64 {y3, y1, true, A, and the split-exact contribution of the last input channel (d3, d1)} of conv over the given operands"""
    xh, xl = split_x(x)
    wh, wl = split_w(w, s)
    sc = 2.0 ** -s
    hh = conv(xh, wh)
    lo = conv(xh, wl) + conv(xl, wh)
    bb = b.double().view(1, -1, 1, 1)
    r = dict(y3=sc * (lo + hh) + bb, y1=sc * hh + bb, true=conv(x.double(), w.double()) + bb,
             A=sc * conv(xh.abs() + xl.abs(), wh.abs() + wl.abs()) + bb.abs())
    c = x.shape[1] - 1                                  # the last channel of the last chunk

    one = lambda a, m: conv(a[:, c:c + 1], m[:, c:c + 1])   # weights: input channels on dim 1 (conv2d layout and the GEMM layout of convT)
    r["d1"] = sc * one(xh, wh)
    r["d3"] = sc * (one(xh, wh) + one(xh, wl) + one(xl, wh))
    return r


def split_reference_3d(x, w, b, s, conv):
    """split_reference for 5-D operands: fp64 {y3, y1, true, A, d3 = split-exact contribution of the last input channel} and, when the
    kernel has three depth taps, z3 = that of the depth tap dz = 0"""
    xh, xl = split_x(x)
    wh, wl = split_w(w, s)
    sc = 2.0 ** -s
    three = lambda ah, al, mh, ml: conv(ah, mh) + conv(ah, ml) + conv(al, mh)
    bb = b.double().view(1, -1, 1, 1, 1)
    hh = conv(xh, wh)
    r = dict(y3=sc * (conv(xh, wl) + conv(xl, wh) + hh) + bb, y1=sc * hh + bb, true=conv(x.double(), w.double()) + bb,
             A=sc * conv(xh.abs() + xl.abs(), wh.abs() + wl.abs()) + bb.abs())
    c = x.shape[1] - 1
    r["d3"] = sc * three(xh[:, c:c + 1], xl[:, c:c + 1], wh[:, c:c + 1], wl[:, c:c + 1])
    if w.shape[2] == 3:
        m = torch.zeros_like(wh)
        m[:, :, 0] = 1.0
        r["z3"] = sc * three(xh, xl, wh * m, wl * m)
    return r


def ratio(got, want, bar):
    return float(((got - want).abs() / bar).max())


def check_stats(out_s, st, B, groups, samples):
    yo = out_s.double()
    n = yo.shape[0]
    want = torch.stack([yo.reshape(n, groups, -1).sum(-1), (yo ** 2).reshape(n, groups, -1).sum(-1)], -1)
    scale = yo.abs().reshape(n, groups, -1).sum(-1)[..., None] + 1.0
    got = st.cpu().view(B, groups, 2)[samples]
    rel = float(((got - want).abs() / scale).max())
    assert rel <= 2e-6, rel


# ---- row Winograd F(2,3) ---------------------------------------------------------------------------------------------------------------
def wino_scale(w):
    """the scale exponent s of pack_conv_weight_wino: max |2^s G w| in [512, 1024)"""
    import math
    G = torch.tensor(WINO_G, dtype=torch.float64)
    umax = float(torch.einsum("pk,ocyk->ocyp", G, w.double()).abs().max())
    s = int(math.floor(math.log2(1024.0 / umax))) if umax > 0 else 0
    return max(-24, min(24, s))


def wino_split_u(w, s):
    """(Uh, Ul) [Cout, Cin, ky, pos] in float64: us = fp32(2^s G w) (G w in fp64), Uh = fp16(us), Ul = fp16(us - Uh)"""
    G = torch.tensor(WINO_G, dtype=torch.float64)
    us = (torch.einsum("pk,ocyk->ocyp", G, w.double()) * (2.0 ** s)).to(torch.float32)
    uh = us.half()
    return uh.double(), (us - uh.float()).half().double()


def wino_split_v(x):
    """(Vh, Vl) [n, C, H, W / 2, pos] in float64: V = fp32(d0 - d2, d1 + d2, d2 - d1, d1 - d3) with d = x[row][2u - 1 .. 2u + 2] (zero outside
    the image), one fp32 operation per value as the kernel's staging does it, then the hi/lo split"""
    assert x.dtype == torch.float32 and x.shape[-1] % 2 == 0
    xp = F.pad(x, (1, 1))
    d0, d1, d2, d3 = xp[..., 0:-2:2], xp[..., 1:-1:2], xp[..., 2::2], xp[..., 3::2]
    v = torch.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], -1)
    vh = v.half()
    return vh.double(), (v - vh.float()).half().double()


def _wino_m(v, u):
    """M_j = sum over (ci, ky) of U_j V_j with zero-padded rows: v [n, C, H, U, 4], u [Cout, C, 3, 4] -> [n, Cout, H, U, 4]"""
    return torch.stack([F.conv2d(v[..., j], u[..., j:j + 1], padding=(1, 0)) for j in range(4)], -1)


def _wino_out(m, signed):
    """output transform: y[2u] = M0 + M1 + M2, y[2u + 1] = M1 - M2 - M3 (signed) or the sum of the same terms (the bound A)"""
    even = m[..., 0] + m[..., 1] + m[..., 2]
    odd = m[..., 1] - m[..., 2] - m[..., 3] if signed else m[..., 1] + m[..., 2] + m[..., 3]
    return torch.stack([even, odd], -1).flatten(-2)


def wino_split_reference(x, w, b, s):
    """As split_reference for the row-Winograd kernel: x [n, C, H, W] fp32 (two inputs concatenated), w [Cout, C, 3, 3], b [Cout] or None.
    y3 = three-term result of the kernel's exact operands in float64, y1 = hi x hi only, true = fp64 convolution of the true operands,
    A = the per-element bound of every partial sum, d3 / d1 = the split-exact contribution of the last input channel."""
    vh, vl = wino_split_v(x)
    uh, ul = wino_split_u(w, s)
    sc = 2.0 ** -s
    bb = (b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)).view(1, -1, 1, 1)
    hh = _wino_m(vh, uh)
    lo = _wino_m(vl, uh) + _wino_m(vh, ul)
    r = dict(y3=sc * _wino_out(hh + lo, True) + bb, y1=sc * _wino_out(hh, True) + bb,
             true=F.conv2d(x.double(), w.double(), padding=1) + bb,
             A=sc * _wino_out(_wino_m(vh.abs() + vl.abs(), uh.abs() + ul.abs()), False) + bb.abs())
    c = x.shape[1] - 1
    one = lambda v, u: _wino_m(v[:, c:c + 1], u[:, c:c + 1])
    r["d1"] = sc * _wino_out(one(vh, uh), True)
    r["d3"] = sc * _wino_out(one(vh, uh) + one(vl, uh) + one(vh, ul), True)
    return r


def wino_unpack(wpk, cout, nchunk):
    """the tensor pack_conv_weight_wino returns -> (hi, lo) [m-tile rows, nchunk * 16, ky, pos] in float64 (the inverse of its fragment
    order [m-tile][chunk][step = ky * 4 + pos][part][h][r][j], channel = chunk * 16 + 8 h + j)"""
    nmt = 4 * ((cout + 127) // 128)
    t = wpk.cpu().view(nmt, nchunk, 12, 2, 2, 32, 8).permute(3, 0, 5, 1, 4, 6, 2).reshape(2, nmt * 32, nchunk * 16, 3, 4)
    return t[0].double(), t[1].double()
