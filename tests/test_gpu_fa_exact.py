"""Every FLASH_ATTN_EXT path against EXACT answers on selector data (tests/fa_exact.py): no tolerance anywhere in this file.

The data makes every probability exactly 0 or exactly 1 / n: integer q, K and V, a power-of-two scale, integer mask values, per query row a tie set
of n = 2^i positions at the maximum and every other live position at least 128 below it.  The one number the design rests on is that gap: expf
underflows to +0 below about -103.98, so exp(-128) is exactly +0 in every kernel, every rescale factor is exactly 0 or 1, and the output is
(sum of the tie set's V rows) / n bit for bit on every path and in every summation order.  fa_exact.exact_expectation asserts the gap (and the other
conditions) on each case's own data; every V row outside the tie sets holds poison.  tests/test_fa_exact_cpu.py holds the same cases against the
CPU restatements and the dispatch rule without a device.

Every case asserts its path first, runs twice and compares the uint32 views of both outputs with the expectation.

  branch                                                        pinned by
  ------------------------------------------------------------  ----------------------------------------------------------------------------
  mnew == -inf inside a live tile (k_flash_attn_mfma)           fused-*-swa, fused-f16-softcap: row 63 of workgroup 0 has tile 1 fully masked
                                                                while row 0 sees it; its later tiles must start from O = 0, sum = 0, alpha = 1
  next_live(0) > 0                                              fused-*-swa (workgroup 0 starts at tile 1, workgroup 1 at tile 2)
  dead tiles in the middle of the walk                          fused-f16-dead_middle, mfma3-*-dead_middle (tiles 1 and 2 dead for all 64 rows;
                                                                they repeat live codes over poison)
  a late, large maximum (alpha = 0 exactly)                     fused-*-late_after_decoy, fused-f16-gqa (a match 128 below in tile 0, the maximum
                                                                in the partial last tile), fused-*-walk (a half-score match in the other tile)
  the P-to-V position permutation, the transposed LDS read      fused-*-walk*: every one of the 64 positions of both tiles is selected by some row,
                                                                every V column chunk (DV = 32, 64, 80) comes from ONE row
  GQA and batch broadcast, ALiBi slopes                         fused-f16-gqa (H = 8 over Hk = 2, B = 2 over Bk = 1, max_bias = 8)
  fam_decode_blk nibble and qh placement, both load forms       fused-<type>-walk-d32 (4-byte aligned), -llama (three one-block heads side by
                                                                side: 2-byte aligned for the 18-, 22- and 34-byte blocks)
  k_flash_attn_combine: the maximum in one piece only           split3-f16-max-piece0 / 1 / 2, split8-f16-kv1025-last-piece (the short piece);
                                                                every other piece holds a match 128 below
  k_flash_attn_combine: a tie set that spans pieces             split3-f16-ties_across-2 / -4, split8-f16-kv1025-mixed
  k_flash_attn_combine: a piece with no live position           split3-f16-piece_dead0 / 2
  bf16 beyond f16's range                                       fused-bf16-big-*: K and V are 2^18 times small integers, the expectation too
  the CPU-following F16 accumulator (seq), the f32 row kernel   seq-f16-mixed, f32-f16-mixed-d80
  the row kernel of a block / bf16 cache                        kvrow-<type>-swa / -late_after_decoy / -ties_across
  tie sets across tiles, up to a whole tile's worth             fused-f16-ties_across-2 / -4 / -64
"""
from types import SimpleNamespace

import numpy as np
import pytest

import fa_exact
from test_fa_exact_cpu import PATHS
from test_gpu_fa_fused import G, torch  # noqa: F401 (fixtures)
from test_gpu_fa_kv import llama_layout


def bits(y):
    return np.ascontiguousarray(y, np.float32).view(np.uint32)


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                             # (a copy: the cases are shared and read-only)


def cache_tensors(torch, c):
    """K and V on the device as the case's layout has them"""
    out = []
    for a in (c.k, c.v):
        if c.cache == "bf16":
            a = a.view(np.int16)                                            # (the bits; viewed as bfloat16 below)
        if c.cache in fa_exact.BLOCK_TYPES:
            out.append(llama_layout(torch, a) if c.run.layout == "heads" else dev(torch, a))
        elif c.run.layout == "heads":                                       # tests/test_gpu_fa_fused.py test_forced_strided_head_views
            buf = dev(torch, np.ascontiguousarray(a[0].transpose(1, 0, 2)))    # [n_kv, Hk, D]
            view = buf.permute(1, 0, 2).unsqueeze(0)
            assert not view.is_contiguous() and view.stride(2) == c.Hk * a.shape[3]
            out.append(view)
        else:
            out.append(dev(torch, a))
        if c.cache == "bf16":
            out[-1] = out[-1].view(torch.int16).view(torch.bfloat16)
    return out


def run_exact(G, torch, monkeypatch, cid, run=None):
    """-> the output; the path asserted first, the call made twice, both outputs equal to the expectation in every bit"""
    c = fa_exact.case(cid)
    run = run or c.run
    if run.fused is None:
        monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    else:
        monkeypatch.setenv("MI355Q_FA_FUSED", run.fused)
    qd, md = dev(torch, c.q), dev(torch, c.mask) if c.mask is not None else None
    kd, vd = cache_tensors(torch, c)
    kv = c.cache if c.cache in fa_exact.BLOCK_TYPES else "q8_0"
    got = G.op_flash_attn_ext_path(qd, kd, vd, md, c.softcap, split=run.split, kv=kv, kv_direct=run.kv_direct)
    assert got == PATHS[run.path], (cid, G.FA_PATH_NAMES.get(got, got))
    ys = [G.op_flash_attn_ext(qd, kd, vd, md, c.scale, c.max_bias, c.softcap, split=run.split, kv=kv, kv_direct=run.kv_direct).cpu().numpy() for _ in range(2)]
    for y in ys:
        bad = bits(y) != bits(c.expect)
        assert not bad.any(), (cid, f"{int(bad.sum())} of {bad.size} elements differ; rows (b, t, h) {sorted(set(zip(*np.nonzero(bad)[:3])))[:8]}")
    return ys[0]


def ids(prefix):
    return [cid for cid in fa_exact.CASES if cid.startswith(prefix)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids("fused-f16-"))
def test_fused_f16(G, torch, monkeypatch, cid):
    run_exact(G, torch, monkeypatch, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids("fused-bf16-"))
def test_fused_bf16_beyond_f16_range(G, torch, monkeypatch, cid):
    y = run_exact(G, torch, monkeypatch, cid)
    assert np.abs(y).max() > 65504


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c for c in ids("fused-") if c.split("-")[1] in fa_exact.BLOCK_TYPES])
def test_fused_on_the_caches_own_rows(G, torch, monkeypatch, cid):
    run_exact(G, torch, monkeypatch, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids("mfma3-"))
def test_three_step_and_fused_agree(G, torch, monkeypatch, cid):
    """the three-step matrix-core path (MI355Q_FA_FUSED=0, with its workspace) and the fused kernel on the same operands: the same bits"""
    c = fa_exact.case(cid)
    y3 = run_exact(G, torch, monkeypatch, cid)
    fused = SimpleNamespace(**dict(vars(c.run), fused="1", path="fused_kv" if c.cache == "bf16" else "fused", kv_direct=c.cache == "bf16"))
    yf = run_exact(G, torch, monkeypatch, cid, run=fused)
    assert np.array_equal(bits(y3), bits(yf))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids("seq-") + ids("split") + ids("f32-"))
def test_row_kernels_f16(G, torch, monkeypatch, cid):
    run_exact(G, torch, monkeypatch, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids("kvrow-"))
def test_kv_row_kernel(G, torch, monkeypatch, cid):
    run_exact(G, torch, monkeypatch, cid)


def test_every_case_is_run():
    run = set(ids("fused-f16-") + ids("fused-bf16-") + [c for c in ids("fused-") if c.split("-")[1] in fa_exact.BLOCK_TYPES] + ids("mfma3-") + ids("seq-")
              + ids("split") + ids("f32-") + ids("kvrow-"))
    assert run == set(fa_exact.CASES)
