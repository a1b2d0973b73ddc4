"""The attention reference of _attention_refs.py against itself, on every row of the table test_gpu_attention_routes.py runs (no GPU):
the fp32 block-wise emulation of each kernel stays under the row's bar, and the bar resolves every near-miss the row answers for.
`pytest -s` prints one line per row: the emulation's ratio and each near-miss as multiples of the bar.  Measured here (CPU, torch's
accumulation order, not the MFMA's): emulation 0.002 - 0.014 of the bar at unit amplitude, 0.05 with q x 8 and on the clamp row; near-misses
qk_lo 5.9 - 16 (1.8 at Nk = 512), v_lo 3.7 - 17 (1.2 at Nk = 512; 13 - 100 with one key), channel 740 - 4.5e5, mask+1 177 - 1.3e5,
mask-1 4.0e3 - 2.1e4, heads 2.7e4 - 1.6e8, rescale 2.4e4 - 1.2e6, clamp 3.0e3."""
import pytest
import torch

from _attention_refs import (BLOCK_ROWS, CLAMP_ROWS, KERNELS, LONG_ROWS, MASK_KERNELS, MASK_NK, MASK_ROWS, RESCALE_ROWS, ROWS, STRIDE_ROWS,
                             WRAPPER_ROWS, attention_refs, emulate, row_refs, worst_ratio)

BY_NAME = {r.name: r for r in ROWS}


def test_the_table_holds_the_rows_it_is_meant_to():
    """every instantiation has its block row; the mask table holds every boundary on the four masked kernels; claims follow the row"""
    assert len(BY_NAME) == len(ROWS) == 74
    assert sorted((r.route, r.d) for r in BLOCK_ROWS) == sorted(KERNELS) and len(KERNELS) == 7
    assert all((r.B, r.heads, r.Nq, r.Nk) == (2, 3, 160, 96) for r in BLOCK_ROWS)
    assert {(r.route, r.d, r.nk_valid) for r in MASK_ROWS if r.Nk == 64} == {(rt, d, nk) for rt, d in MASK_KERNELS for nk in MASK_NK}
    assert {(r.route, r.d) for r in MASK_ROWS if r.Nk == 32 and r.nk_valid == 1} == set(MASK_KERNELS) and len(MASK_ROWS) == 48
    assert {(r.route, r.d) for r in STRIDE_ROWS} == {(0, 8), (1, 32)}
    assert {(r.route, r.d, r.kind) for r in RESCALE_ROWS} == {(rt, d, kd) for rt, d in ((1, 64), (0, 8)) for kd in ("asc", "desc", "q8")}
    assert all((r.B, r.heads, r.Nq, r.Nk) == (1, 2, 32, 512) for r in LONG_ROWS) and {(r.route, r.d) for r in LONG_ROWS} == {(1, 64), (0, 8)}
    assert [(r.route, r.d) for r in CLAMP_ROWS] == [(1, 32)] and len(WRAPPER_ROWS) == 8
    for r in ROWS:
        assert r.misv == (r.route == 0 and r.d >= 16) and (r.route == 1) <= (r.d >= 16)
        assert r.Nq % 32 == 0 and r.Nk % 32 == 0 and r.Nk - 32 < r.nk_valid <= r.Nk, r
        assert ("heads" in r.claims) == (r.B > 1), r
        masked = r.nk_valid < r.Nk
        assert ("mask+1" in r.claims) == masked and ("mask-1" in r.claims) == (masked and r.nk_valid > 1), r
        assert ("channel" in r.claims) == (r.nk_valid > 1), r
        if r.route == 0:
            assert not {"qk_lo", "v_lo"} & set(r.claims), r
        elif r in BLOCK_ROWS + MASK_ROWS + STRIDE_ROWS + LONG_ROWS + WRAPPER_ROWS:
            assert "v_lo" in r.claims and ("qk_lo" in r.claims) == (r.nk_valid > 1), r
    assert all("rescale" in r.claims for r in RESCALE_ROWS if r.kind != "desc") and "clamp" in CLAMP_ROWS[0].claims


@pytest.mark.parametrize("name", list(BY_NAME))
def test_emulation_stays_under_the_bar_and_the_bar_resolves_the_near_misses(name):
    row = BY_NAME[name]
    (q, k, v), r = row_refs(row)
    y, bar = r["y"], r["bar"]
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(bar).all()) and bool((bar > 0).all())
    emu = worst_ratio(emulate(q, k, v, row.heads, row.nk_valid, row.route), y, bar)
    near = {c: worst_ratio(t, y, bar) for c, t in r["near"].items()}
    print("\n  %-26s route %d  emulation %.4f  %s" % (row.name, row.route, emu, "  ".join("%s %.3g" % kv for kv in near.items())))
    assert emu <= 1.0, "%s: the fp32 emulation of the kernel is at %.3f x the bar" % (name, emu)
    assert set(near) == set(row.claims)
    for c, x in near.items():
        assert x > 1.0, "%s: the bar does not resolve the near-miss %r (%.3f x the bar)" % (name, c, x)
    if row.unit:
        assert float((y - r["true"]).abs().max()) <= 2e-6, "the reference itself is a tenth of the standing 2e-5 from the true result"


def test_reference_is_plain_attention_on_exact_operands():
    """operands exactly representable in f16 whose scaled q is exact too (d = 16: 1 / 4): both routes' references are the fp64 attention of
    the true operands, masked or not; with nk_valid = 1 the output is that key's V row whatever the scores are"""
    B, heads, d, Nq, Nk = 2, 3, 16, 32, 64
    g = torch.Generator().manual_seed(5)
    mk = lambda n: (torch.randint(-8, 9, (B, heads * d, n), generator=g).float() / 8.0)      # noqa: E731
    q, k, v = mk(Nq), mk(Nk), mk(Nk)
    for route in (0, 1):
        for nk in (64, 45, 33):
            r = attention_refs(q, k, v, heads, nk, route)
            assert float((r["y"] - r["true"]).abs().max()) <= 1e-15, (route, nk)
        r = attention_refs(q, k[:, :, :32].contiguous(), v[:, :, :32].contiguous(), heads, 1, route)
        want = v[:, :, :1].double().expand(B, heads * d, Nq)
        assert torch.equal(r["y"], want) and torch.equal(r["true"], want)

