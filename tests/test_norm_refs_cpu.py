"""The references of tests/_norm_refs.py, checked without a GPU: pinned to torch's own float64 normalisations at 1e-12 (so helper and kernel
cannot be wrong together), an fp32 emulation of every kernel expression held to the bar of every GPU row (the reference alone stays inside),
and every near-miss reference beyond it on the rows that name it.  pytest -s prints the worst ratios (profiles/norm_route_table.md)."""
import math

import pytest
import torch
import torch.nn.functional as F

import _norm_refs as R

_ids = lambda rows: [r.name for r in rows]
TORCH_ACT = {"none": lambda t: t, "gelu": F.gelu, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, R.SLOPE), "tanh": torch.tanh, "sigmoid": torch.sigmoid}


def close(a, b, tol=1e-12):
    return float(((a - b).abs() / b.abs().clamp_min(1.0)).max()) <= tol


@pytest.mark.parametrize("row", R.APPLY_ROWS, ids=_ids(R.APPLY_ROWS))
def test_apply_reference_is_torch_group_norm(row):
    inp = R.apply_inputs(row)
    x4 = inp["x"].double().view(row.B, row.C, row.HW, 1)
    for form in R.forms_of(row):
        kw = R.form_kwargs(inp, form)
        ref, _ = R.apply_refs(inp["x"], inp["ws"], groups=row.groups, **kw)
        dd = lambda p: None if p is None else p.double()
        y = F.group_norm(x4, row.groups, dd(kw["gamma"]), dd(kw["beta"]), R.EPS).view(row.B, row.C, row.HW)
        r = 0.0
        if kw.get("res_mode"):
            r = kw["res"].double()
            if "res_norm" in kw:
                r = F.group_norm(r.view(x4.shape), row.groups, inp["gamma_r"].double(), inp["beta_r"].double(), R.EPS).view(y.shape)
        want = TORCH_ACT[kw["act"]](y + r) if kw.get("res_mode") == "before_act" else TORCH_ACT[kw["act"]](y) + r
        # E[x^2] - E[x]^2 of the fp64 sums against torch's two-pass variance: 2^-52 (1 + mean^2 / var), 1e-12 of the output at mean / std = 64
        assert close(ref, want, 1e-12 if row.data == "std" else 4e-12), (row.name, form)


def test_instance_norm_is_the_groups_equal_channels_case():
    x = R.make_data("std", (3, 6, 50), seed=1)
    ref, _ = R.apply_refs(x, R.host_ws(x, 6), None, None, 6)
    assert close(ref, F.instance_norm(x.double(), eps=R.EPS))


@pytest.mark.parametrize("row", R.LN_ROWS, ids=_ids(R.LN_ROWS))
def test_layer_norm_reference_emulation_and_near_misses(row):
    inp = R.ln_inputs(row)
    ref, bar = R.ln_refs(**inp)
    want = F.layer_norm(inp["x"].double().transpose(1, 2), (row.C,), inp["gamma"].double(), inp["beta"].double(), R.EPS).transpose(1, 2)
    assert close(ref, want, 1e-12 if row.data == "std" else 4e-12)
    emu = R.ratio(R.emulate_ln(**inp), ref, bar)
    near = {}
    if row.C > 1:
        near = {"C-1": R.ratio(R.ln_refs(bessel=True, **inp)[0], ref, bar), "no-last-channel": R.ratio(R.ln_refs(drop_last=True, **inp)[0], ref, bar)}
    else:
        assert torch.equal(R.emulate_ln(**inp), inp["beta"].float().view(1, 1, 1).expand(row.B, 1, row.N))      # x - mean is exactly 0
    print("\n  ln %-24s emulation %.3f  %s" % (row.name, emu, "  ".join("%s %.3g" % kv for kv in near.items())))
    assert emu <= 1.0 and all(v > 1.0 for v in near.values()), (emu, near)


def test_activation_references_and_sweep():
    dense, tail = R.sweep_inputs()
    v = torch.cat([dense, tail])
    assert close(R.act64(v.double(), "gelu"), F.gelu(v.double()))
    for act in R.ACTS:
        ref, bar = R.sweep_refs(v, act)
        assert close(ref, TORCH_ACT[act](v.double()), 1e-12 if act != "lrelu" else 2.0 ** -23)
        got = R.act_f32(v, act)
        worst = R.ratio(got, ref, bar)
        print("\n  sweep %-8s emulation %.3f" % (act, worst))
        assert worst <= 1.0, act
    ref, bar = R.sweep_refs(v, "gelu")
    tanh_form = R.ratio(R.gelu_tanh64(v.double()), ref, bar)
    print("\n  sweep gelu: tanh form %.3g x the bar" % tanh_form)
    assert tanh_form > 1.0


@pytest.mark.parametrize("row", R.STATS_ROWS, ids=_ids(R.STATS_ROWS))
def test_statistics_emulation_and_near_misses(row):
    c = R.stats_case(row)
    x = c["x"]
    if row.plan[0] == 1:
        emu = R.emulate_block_stats(x, row.groups)
    else:                                                          # the wave kernel's order: 64 lane sums in fp64, then their sum
        v = x.double().reshape(row.B, row.groups, -1)
        v = F.pad(v, (0, -v.shape[-1] % 64)).view(row.B, row.groups, -1, 64)
        emu = torch.stack([v.sum(2).sum(-1), (v * v).sum(2).sum(-1)], -1)
    r = R.ratio(emu, c["ref"], c["bar"])
    near = {k: R.ratio(v, c["ref"], c["bar"]) for k, v in c["near"].items()}
    assert set(near) == set(row.near)
    relvar = float(((R.variance_of(emu, c["L"]) - R.variance_of(c["ref"], c["L"])).abs() / R.variance_of(c["ref"], c["L"])).max())
    print("\n  stats %-24s emulation %.4f  relative variance error %.2e  %s" % (row.name, r, relvar, "  ".join("%s %.3g" % kv for kv in near.items())))
    assert r <= 1.0 and all(v > 1.0 for v in near.values()), (r, near)


def test_block_statistics_presums_lose_the_variance_of_offset_data():
    """what the bar of the block route means for E[x^2] - E[x]^2: the emulation at mean / std = 64 and 1000"""
    for mean, L in ((64.0, 8192), (1000.0, 65536)):
        x = (mean + R.randn(1, 1, L, seed=7)).float()
        ref = R.host_ws(x, 1)
        emu = R.emulate_block_stats(x, 1)
        rel = float((R.variance_of(emu, L) - R.variance_of(ref, L)).abs() / R.variance_of(ref, L))
        print("\n  block statistics, mean / std %g, L %d: relative variance error %.2e" % (mean, L, rel))
        assert rel <= 2.0 ** -22 * (mean * mean + 1) * 2.2          # dSS / L + 2 |mean| dS / L over var, from the two bars
        assert R.ratio(emu, ref, torch.stack([x.double().abs().sum() * 2.0 ** -23, (x.double() ** 2).sum() * 2.0 ** -22]).view(1, 1, 2)) <= 1.0


@pytest.mark.parametrize("row", R.APPLY_ROWS, ids=_ids(R.APPLY_ROWS))
def test_apply_emulation_and_near_misses(row):
    inp = R.apply_inputs(row)
    for form in R.forms_of(row):
        kw = R.form_kwargs(inp, form)
        ref, bar = R.apply_refs(inp["x"], inp["ws"], groups=row.groups, **kw)
        emu = R.ratio(R.emulate_apply(inp["x"], inp["ws"], groups=row.groups, **kw), ref, bar)
        near = R.apply_near_misses(row, inp, form, ref, bar)
        print("\n  apply %-26s %-20s emulation %.3f  %s" % (row.name, form, emu, "  ".join("%s %.3g" % kv for kv in near.items())))
        assert emu <= 1.0, (row.name, form, emu)
        assert "neighbour-slab" in near and all(v > 1.0 for v in near.values()), (row.name, form, near)
        if row.data == "smallvar":
            assert near["eps/10"] > 1000 and near["eps=0"] > 1000


@pytest.mark.parametrize("row", [r for r in R.APPLY_ROWS if r.name in ("small-vec-one-short-block", "large-vec-asegs1")], ids=lambda r: r.name)
def test_constant_slab_gives_beta_bitwise(row):
    inp = R.constant_slab_inputs(row)
    out = R.emulate_apply(inp["x"], inp["ws"], inp["gamma"], inp["beta"], row.groups)
    cpg = row.C // row.groups
    for slab in (0, 1):
        b, g = divmod(slab, row.groups)
        want = inp["beta"].float()[g * cpg:(g + 1) * cpg, None].expand(cpg, row.HW)
        assert torch.equal(out[b, g * cpg:(g + 1) * cpg], want)
    ref, bar = R.apply_refs(inp["x"], inp["ws"], inp["gamma"], inp["beta"], row.groups)
    assert R.ratio(out, ref, bar) <= 1.0


@pytest.mark.parametrize("row", R.COEF_ROWS, ids=_ids(R.COEF_ROWS))
def test_coef_emulation(row):
    inp = R.coef_inputs(row)
    rm, rs, same = R.coef_ratios(R.emulate_coef(row, inp), *R.coef_refs(row, inp))
    print("\n  coef %-22s mean %.3f scale %.3f" % (row.name, rm, rs))
    assert rm <= 1.0 and rs <= 1.0 and same


@pytest.mark.parametrize("row", R.HEAD_ROWS, ids=_ids(R.HEAD_ROWS))
def test_head_emulation_and_near_misses(row):
    inp = R.head_inputs(row)
    ref, bar = R.head_refs(slope=row.slope, **inp)
    emu = R.ratio(R.emulate_head(slope=row.slope, **inp), ref, bar)
    near = {"no-last-channel": R.ratio(R.head_refs(slope=row.slope, drop_last=True, **inp)[0], ref, bar),
            "other-slope": R.ratio(R.head_refs(slope=0.01 - row.slope, **inp)[0], ref, bar)}
    print("\n  head %-26s emulation %.3f  %s" % (row.name, emu, "  ".join("%s %.3g" % kv for kv in near.items())))
    assert emu <= 1.0 and all(v > 1.0 for v in near.values()), (emu, near)


def test_head_reference_is_norm_lrelu_conv():
    row = R.HEAD_ROWS[1]
    inp = R.head_inputs(row)
    ref, _ = R.head_refs(slope=row.slope, **inp)
    c = inp["coef"].double()
    t = F.leaky_relu((inp["x"].double() - c[:, 0, :, None]) * c[:, 1, :, None] + c[:, 2, :, None], R.SLOPE)
    assert close(ref, F.conv1d(t, inp["w"].double()[:, :, None], None if inp["bias"] is None else inp["bias"].double()))
    assert not math.isnan(float(ref.sum()))
