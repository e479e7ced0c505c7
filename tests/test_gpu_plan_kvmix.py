"""The decode plan's attention stage over MIXED K / V cache types (mi355q_stage.flags MI355Q_STAGE_KV_* for K with a MI355Q_STAGE_KVV_* bit for V;
`-fa 1 -ctk A -ctv B`, A != B among f16, q8_0, q4_0, q4_1, q5_0, q5_1, iq4_nl), regs engine, in the pattern of tests/test_gpu_plan_kvq.py: a Q4_K GEMV
stage produces q, k and v, then the attention stage runs.

What is compared with what:
  * the rows the stage stores for this token: byte for byte against mi355q_op_cpy of the device's own roped k (into K's type) and of v (into V's type);
    every other cache row is left as it was (all 42 pairs);
  * the output with one KV split: bit for bit against mi355q_op_flash_attn_ext2 with MI355Q_FA_KV_MIXED on the same cache AND against
    tests/kvmix_ref.py (pinned to the reference by tests/test_kvmix_ref_cpu.py);
  * several splits (windows above 256 positions) against the restatement: a block V within SPLIT_BOUND = 8e-7 of max|ref| (the block stages' bound,
    tests/test_gpu_plan_kvq.py); an f16 V within F32_BOUND = 2e-5, the bound tests/test_gpu_plan_attn_forms.py holds the f16 stage's
    several-split form to.  The CPU check of those bounds (kvmix_ref evaluated per split and merged in float64) was NOT made on this file's own q / K / V:
    q comes out of the device's GEMV stage.  It was made on unit-variance q / K / V (8 heads of 128 over 2 kv heads, windows of 512 and 1024: a flat
    softmax, the hardest case for a merge), where the reference's own split-and-merge is 0.7e-6 .. 1.8e-6 of max|ref| for the six block-V RING pairs --
    ABOVE SPLIT_BOUND, so 8e-7 is not confirmed on the CPU for the data used here and rests on the device figures below, on this file's peaked
    softmaxes, and on the same-type stages' record with the same bound and data -- and 5.5e-3 .. 9.1e-3 for (iq4_nl, f16), F16 or f32 partials alike:
    the distance of ANY merge from the CPU's single F16-accumulator walk is that walk's own rounding chain (2^-11 per position), and a stage that merged
    f32 partials measured 1.7e-4 / 2.4e-4 on this file's data.  So an f16 V is not merged: its splits score in parallel and then CONTINUE one walk, split
    after split (plan_attn_mix step 3b), which is the CPU's walk itself -- the error against the restatement is 0.  With this file's data (q out of the
    GEMV stage: a peaked softmax) the block-V pairs measured 3.2e-8 .. 1.8e-7 of max|ref| on an MI355X;
  * a V bit equal to K's type: the flag-less same-type stage, bit for bit, output and stores;
  * a 24-token decode loop against the node ops (op_rope -> op_cpy_indirect -> op_flash_attn_ext mixed) on a twin cache: the same bits at every step;
  * refused at plan creation, nothing launched: a window past the pair's LDS limit (the message gives the limit), head sizes that are not whole blocks,
    the transposed V layout, two V bits, bf16, the ring engine.
Never-written cache rows beyond the token hold NaN (a block side: NaN scales; an f16 side: NaN elements): a masked position must not be read.
"""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import kvmix_ref
import oracle
from conftest import PKG, ROOT
from qdata import quantized_weights

pytestmark = pytest.mark.gpu

TYPES = list(kvmix_ref.TYPES)
PAIRS = [(kt, vt) for kt in TYPES for vt in TYPES if kt != vt]
RING = list(kvmix_ref.RING)
BB = {t: kvmix_ref.BLOCK_BYTES[t] for t in TYPES}                                # bytes per 32 elements of a row (f16: 64)
SPLIT_BOUND = 8e-7                                                               # a block V, several splits (tests/test_gpu_plan_kvq.py)
F32_BOUND = 2e-5                                                                 # an f16 V, several splits (tests/test_gpu_plan_attn_forms.py)
ids = lambda p: f"{p[0]}-{p[1]}"


@pytest.fixture(scope="module")
def G():
    import torch
    import ggml_mi355 as g
    assert torch.cuda.is_available() and g.lib().mi355q_device_count() >= 1
    return g


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def W(G, t, m, k, rng):
    return G.QWeight.from_host(t, quantized_weights(t, m, k, rng), m, k)


def store_rows(G, torch, x, t):
    """op_cpy f32 [n, m] -> the side's rows as bytes, uint8 [n, m / 32 * BB] on the device."""
    if t == "f16":
        out = torch.zeros(x.shape, dtype=torch.float16, device="cuda")
        G.op_cpy(x, out)
        return out.view(torch.uint8)
    out = torch.zeros((x.shape[0], x.shape[1] // 32 * BB[t]), dtype=torch.uint8, device="cuda")
    G.op_cpy(x, out, kv=t)
    return out


def poison(cache_np, rows, t):
    """NaN in the given rows (never-written cache cells): a block side through its f16 scales, an f16 side in every element."""
    c = cache_np.copy()
    if t == "f16":
        c[rows] = np.tile(np.array([0x00, 0x7E], np.uint8), c.shape[1] // 2)
    else:
        c.reshape(c.shape[0], c.shape[1] // BB[t], BB[t])[rows, :, 0:2] = np.array([0x00, 0x7E], np.uint8)          # f16 NaN, little endian
    return c


def side(t, torch_mod, c):
    """a cache's bytes as op_flash_attn_ext wants the side: f16 tensor or uint8 block rows"""
    return c.view(torch_mod.float16) if t == "f16" else c


class Stage:
    """A GEMV stage producing q / k / v, then the attention stage over a K cache of type kt and a V cache of type vt, on random inputs."""

    def __init__(self, G, torch, kt, vt, n_head, n_head_kv, hd, n_kv, pos, mask_kind="f16", mode=0, seed=0, E=256, kv_v="auto"):
        rng = np.random.default_rng(seed)
        self.G, self.torch, self.kt, self.vt = G, torch, kt, vt
        self.n_head, self.n_head_kv, self.hd, self.n_kv, self.pos, self.mode = n_head, n_head_kv, hd, n_kv, pos, mode
        n_q, n_k = n_head * hd, n_head_kv * hd
        self.krb, self.vrb = hd // 32 * BB[kt], hd // 32 * BB[vt]
        self.krow, self.vrow = n_head_kv * self.krb, n_head_kv * self.vrb      # bytes per cache position
        n_ctx = n_kv + 32
        wq, wk, wv = W(G, oracle.Q4_K, n_q, E, rng), W(G, oracle.Q4_K, n_k, E, rng), W(G, oracle.Q4_K, n_k, E, rng)
        x = dev(torch, rng.standard_normal((1, E)).astype(np.float32))
        self.q, self.k, self.v = (torch.zeros((1, n), dtype=torch.float32, device="cuda") for n in (n_q, n_k, n_k))
        self.out = torch.zeros((1, n_q), dtype=torch.float32, device="cuda")
        kc = store_rows(G, torch, dev(torch, rng.standard_normal((n_ctx, n_k)).astype(np.float32)), kt).cpu().numpy()
        vc = store_rows(G, torch, dev(torch, rng.standard_normal((n_ctx, n_k)).astype(np.float32)), vt).cpu().numpy()
        self.kc_h, self.vc_h = poison(kc, slice(pos + 1, None), kt), poison(vc, slice(pos + 1, None), vt)
        self.kc, self.vc = dev(torch, self.kc_h), dev(torch, self.vc_h)
        if mask_kind is None:
            assert n_kv == pos + 1                                        # (no mask: the window is exactly the written positions)
            self.mask_h = None; mask = None
        else:
            self.mask_h = np.full(n_kv, -np.inf, np.float32)
            self.mask_h[:pos + 1] = rng.choice(np.array([0.0, 0.0, -0.5, -1.25], np.float32), pos + 1)   # (values exact in f16)
            mask = dev(torch, self.mask_h if mask_kind == "f32" else self.mask_h.astype(np.float16))
        self.posd = dev(torch, np.array([pos], np.int32))
        self.dst = torch.tensor([self.kc.data_ptr() + pos * self.krow, self.vc.data_ptr() + pos * self.vrow], dtype=torch.int64, device="cuda")
        self.scale = 1.0 / np.sqrt(hd)
        self.attn = dict(q=self.q, k=self.k, v=self.v, pos=self.posd, rope=dict(n_dims=hd, mode=mode, n_ctx_orig=8192, freq_base=500000.0),
                         k_cache=self.kc, v_cache=self.vc, k_nb_pos=self.krow, k_nb_head=self.krb, v_nb_pos=self.vrow, v_nb_dim=2 if vt == "f16" else BB[vt],
                         v_nb_head=self.vrb, k_dst=self.dst[0:1], v_dst=self.dst[1:2], v_dst_nb=2 if vt == "f16" else 0, mask=mask, n_head=n_head,
                         n_head_kv=n_head_kv, head_dim=hd, n_kv=n_kv, scale=self.scale, out=self.out, kv=kt)
        if kv_v == "auto":
            self.attn["kv_v"] = vt
        elif kv_v is not None:
            self.attn["kv_v"] = kv_v
        self.stages = [dict(ws=[wq, wk, wv], ys=[self.q, self.k, self.v], x=x), dict(attn=self.attn)]

    def run(self):
        plan = self.G.Plan(self.stages)
        plan.run(); self.torch.cuda.synchronize()
        assert plan.status() == 0
        plan.close()

    def rope(self, t, n):
        return self.G.op_rope(t.view(1, 1, n, self.hd), self.posd, self.hd, self.mode, n_ctx_orig=8192, freq_base=500000.0)

    def check_stores(self):
        """The stored rows are op_cpy of the device's roped k (K's type) / of v (V's type); nothing else changed.  Returns the caches as they now are."""
        torch, n_k = self.torch, self.n_head_kv * self.hd
        k_r = self.rope(self.k, self.n_head_kv).reshape(1, n_k)
        want_k = store_rows(self.G, torch, k_r, self.kt).cpu().numpy()[0]
        want_v = store_rows(self.G, torch, self.v, self.vt).cpu().numpy()[0]
        kc, vc = self.kc.cpu().numpy(), self.vc.cpu().numpy()
        assert np.array_equal(kc[self.pos], want_k), "stored K row"
        assert np.array_equal(vc[self.pos], want_v), "stored V row"
        other = np.ones(kc.shape[0], bool); other[self.pos] = False
        assert np.array_equal(kc[other], self.kc_h[other]) and np.array_equal(vc[other], self.vc_h[other]), "other cache rows changed"
        return kc, vc

    def windows(self, kc, vc):
        """[1, n_head_kv, n_kv, row bytes] uint8 of each side"""
        wk = kc[:self.n_kv].reshape(self.n_kv, self.n_head_kv, self.krb).transpose(1, 0, 2)[None]
        wv = vc[:self.n_kv].reshape(self.n_kv, self.n_head_kv, self.vrb).transpose(1, 0, 2)[None]
        return np.ascontiguousarray(wk), np.ascontiguousarray(wv)

    def reference(self, kc, vc):
        """kvmix_ref.flash_attn_ext on the device's roped q and the cache as stored -> [n_head, hd] f32.  (Masked rows hold NaN: zeroed for numpy's sake,
        the restatement skips them as the CPU does.)"""
        q_r = self.rope(self.q, self.n_head).cpu().numpy().reshape(1, self.n_head, 1, self.hd)
        wk, wv = self.windows(kc, vc)
        mask = None if self.mask_h is None else self.mask_h.reshape(1, self.n_kv)
        if mask is not None:
            dead = ~np.isfinite(self.mask_h)
            wk[:, :, dead] = 0; wv[:, :, dead] = 0
        with np.errstate(all="ignore"):
            return kvmix_ref.flash_attn_ext(self.kt, self.vt, q_r, wk, wv, mask, self.scale).reshape(self.n_head, self.hd)

    def node_op(self, kc, vc):
        """mi355q_op_flash_attn_ext2 (MI355Q_FA_KV_MIXED) on the device's roped q and the same cache -> [n_head, hd] f32."""
        G, torch = self.G, self.torch
        q_r = self.rope(self.q, self.n_head).view(1, self.n_head, 1, self.hd)
        wk, wv = self.windows(kc, vc)
        mask = None if self.mask_h is None else dev(torch, self.mask_h.astype(np.float16).reshape(1, self.n_kv))
        o = G.op_flash_attn_ext(q_r, side(self.kt, torch, dev(torch, wk)), side(self.vt, torch, dev(torch, wv)), mask, float(self.scale),
                                kv=self.kt if self.kt != "f16" else "q8_0", kv_v=self.vt if self.vt != "f16" else None, kv_mixed=True)
        return o.cpu().numpy().reshape(self.n_head, self.hd)

    def got(self):
        return self.out.cpu().numpy().reshape(self.n_head, self.hd)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_one_split(st):
    st.run()
    kc, vc = st.check_stores()
    got, ref = st.got(), st.reference(kc, vc)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(ref)), ("restatement", np.abs(got - ref).max())
    assert np.array_equal(bits(got), bits(st.node_op(kc, vc))), "node op"


SMALL = (4, 2, 64, 64, 40, 2)                                                    # n_head, n_head_kv, head_dim, n_kv, pos, rope mode (neox)


@pytest.mark.parametrize("pair", PAIRS, ids=ids)
def test_small_shape_stores_and_one_split_bits(G, torch, pair):
    """All 42 pairs: the stored rows (check_stores) and the output bits, two kv heads of 64 under neox rope."""
    n_head, n_head_kv, hd, n_kv, pos, mode = SMALL
    check_one_split(Stage(G, torch, pair[0], pair[1], n_head, n_head_kv, hd, n_kv, pos, "f16", mode, seed=zlib.crc32(ids(pair).encode()) % 1000))


@pytest.mark.parametrize("pair", RING, ids=ids)
def test_three_blocks_per_row_no_gqa(G, torch, pair):
    check_one_split(Stage(G, torch, pair[0], pair[1], 8, 8, 96, 128, 100, "f16", 0, seed=zlib.crc32(ids(pair).encode()) % 1000 + 1))


LLAMA = [("q8_0", "q4_0"), ("f16", "q8_0"), ("q8_0", "f16")]


@pytest.mark.parametrize("pair", LLAMA, ids=ids)
def test_llama_8b_shape(G, torch, pair):
    check_one_split(Stage(G, torch, pair[0], pair[1], 32, 8, 128, 256, 200, "f16", 0, seed=7))


@pytest.mark.parametrize("mask", ["f32", "f16", None], ids=["mask_f32", "mask_f16", "no_mask"])
@pytest.mark.parametrize("pair", [("q8_0", "q4_0"), ("f16", "q5_1"), ("q4_1", "f16")], ids=ids)
def test_mask_kinds(G, torch, pair, mask):
    n_head, n_head_kv, hd, n_kv, pos, mode = SMALL
    check_one_split(Stage(G, torch, pair[0], pair[1], n_head, n_head_kv, hd, pos + 1 if mask is None else n_kv, pos, mask, mode, seed=13))


@pytest.mark.parametrize("pair", RING, ids=ids)
def test_forced_single_split_of_512(G, torch, pair, monkeypatch):
    """The longest single-split walk that still takes seconds: MI355Q_PLAN_KV_SPLIT=1 over a window of 512.  Heads of 64: with an f16 side at
    head_dim 128 one split holds at most 384 positions (256 + 136 + 8 bytes each for (f16, q8_0)), and every RING pair runs the same shape."""
    monkeypatch.setenv("MI355Q_PLAN_KV_SPLIT", "1")
    check_one_split(Stage(G, torch, pair[0], pair[1], 32, 8, 64, 512, 450, "f16", seed=3))


@pytest.mark.parametrize("n_kv", [512, 1024])
@pytest.mark.parametrize("pair", RING, ids=ids)
def test_several_splits_within_the_bound(G, torch, pair, n_kv, monkeypatch, capfd):
    """2 and 4 splits at the 8B head shape against the restatement.  The split count is plan_create's own (one per 256 positions, at most #CU / n_head):
    read back from its verbose line, and the case is void unless more than one split ran."""
    monkeypatch.delenv("MI355Q_PLAN_KV_SPLIT", raising=False)
    monkeypatch.setenv("MI355Q_PLAN_VERBOSE", "1")
    st = Stage(G, torch, pair[0], pair[1], 32, 8, 128, n_kv, n_kv - 7, "f16", seed=n_kv % 97)
    capfd.readouterr()
    st.run()
    m = re.search(rf"attention stage \d+: n_kv {n_kv}, (\d+) split\(s\) of (\d+) positions, {pair[0]} / {pair[1]} cache", capfd.readouterr().err)
    assert m, "no verbose line of the mixed stage"
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert int(m.group(1)) == min((n_kv + 255) // 256, n_cu // 32) and int(m.group(1)) > 1, m.group(0)
    kc, vc = st.check_stores()
    got, ref = st.got(), st.reference(kc, vc)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
    bound = F32_BOUND if pair[1] == "f16" else SPLIT_BOUND
    print(f"{ids(pair)} n_kv {n_kv}: max error {err:.3e} of max|out| (bound {bound:.0e})")
    assert err <= bound, err


@pytest.mark.parametrize("kv", ["q8_0", "q4_1"])
def test_v_bit_equal_to_k_is_the_same_type_stage(G, torch, kv):
    n_head, n_head_kv, hd, n_kv, pos, mode = SMALL
    res = []
    for kv_v in (None, kv):
        st = Stage(G, torch, kv, kv, n_head, n_head_kv, hd, n_kv, pos, "f16", mode, seed=21, kv_v=kv_v)
        assert ("kv_v" in st.attn) == (kv_v is not None)
        st.run()
        res.append((st.got().copy(), *st.check_stores()))
    assert np.array_equal(bits(res[0][0]), bits(res[1][0]))
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("pair", [("q8_0", "q4_0"), ("f16", "q8_0"), ("q5_1", "f16")], ids=ids)
def test_decode_loop_matches_the_node_ops(G, torch, pair):
    """24 tokens through ONE plan whose K / V destinations move every token, against op_rope -> op_cpy_indirect -> op_flash_attn_ext (mixed) on a twin
    cache; the window (n_kv_dev, padded to 32 as the plugin pads it) grows across a 32-position boundary."""
    kt, vt = pair
    n_head, n_head_kv, hd, n_ctx, p0 = 8, 2, 128, 96, 50
    rng = np.random.default_rng(11)
    n_q, n_k = n_head * hd, n_head_kv * hd
    krb, vrb = hd // 32 * BB[kt], hd // 32 * BB[vt]; krow, vrow = n_head_kv * krb, n_head_kv * vrb
    q, k, v = (torch.zeros((1, n), dtype=torch.float32, device="cuda") for n in (n_q, n_k, n_k))
    out = torch.zeros((1, n_q), dtype=torch.float32, device="cuda")
    kc1 = dev(torch, poison(store_rows(G, torch, dev(torch, rng.standard_normal((n_ctx, n_k)).astype(np.float32)), kt).cpu().numpy(), slice(p0, None), kt))
    vc1 = dev(torch, poison(store_rows(G, torch, dev(torch, rng.standard_normal((n_ctx, n_k)).astype(np.float32)), vt).cpu().numpy(), slice(p0, None), vt))
    kc2, vc2 = kc1.clone(), vc1.clone()                                           # node ops
    mask_h = np.full(n_ctx, -np.inf, np.float16)
    mask = dev(torch, mask_h)
    posd = dev(torch, np.array([p0], np.int32))
    nkv = dev(torch, np.array([64], np.int32))
    dst = torch.tensor([kc1.data_ptr() + p0 * krow, vc1.data_ptr() + p0 * vrow], dtype=torch.int64, device="cuda")
    table = torch.tensor([kc2.data_ptr() + p0 * krow, vc2.data_ptr() + p0 * vrow], dtype=torch.int64, device="cuda")
    scale = 1.0 / np.sqrt(hd)
    w0 = W(G, oracle.Q4_K, 32, 256, rng); x0 = torch.zeros((1, 256), dtype=torch.float32, device="cuda"); y0 = torch.zeros((1, 32), dtype=torch.float32, device="cuda")
    attn = dict(q=q, k=k, v=v, pos=posd, rope=dict(n_dims=hd, mode=0, n_ctx_orig=8192, freq_base=500000.0), k_cache=kc1, v_cache=vc1,
                k_nb_pos=krow, k_nb_head=krb, v_nb_pos=vrow, v_nb_dim=2 if vt == "f16" else BB[vt], v_nb_head=vrb, k_dst=dst[0:1], v_dst=dst[1:2],
                v_dst_nb=2 if vt == "f16" else 0, mask=mask, n_head=n_head, n_head_kv=n_head_kv, head_dim=hd, n_kv=n_ctx, n_kv_dev=nkv, scale=scale, out=out,
                kv=kt, kv_v=vt)
    plan = G.Plan([([w0], x0, [y0], False), dict(attn=attn)])
    k_view = torch.zeros((1, n_k), dtype=torch.float16, device="cuda") if kt == "f16" else torch.zeros((1, krow), dtype=torch.uint8, device="cuda")
    v_view = torch.zeros((1, n_k), dtype=torch.float16, device="cuda") if vt == "f16" else torch.zeros((1, vrow), dtype=torch.uint8, device="cuda")
    windows = set()
    for step in range(24):
        p = p0 + step
        w = (p + 1 + 31) // 32 * 32                                               # 64 up to position 63, then 96
        windows.add(w)
        for t in (q, k, v):
            t.copy_(dev(torch, rng.standard_normal(t.shape).astype(np.float32)))
        posd.fill_(p); nkv.fill_(w)
        mask_h[:p + 1] = 0.0
        mask.copy_(dev(torch, mask_h))
        dst.copy_(torch.tensor([kc1.data_ptr() + p * krow, vc1.data_ptr() + p * vrow], dtype=torch.int64))
        table.copy_(torch.tensor([kc2.data_ptr() + p * krow, vc2.data_ptr() + p * vrow], dtype=torch.int64))
        plan.run()
        q_r = G.op_rope(q.view(1, 1, n_head, hd), posd, hd, 0, n_ctx_orig=8192, freq_base=500000.0)
        k_r = G.op_rope(k.view(1, 1, n_head_kv, hd), posd, hd, 0, n_ctx_orig=8192, freq_base=500000.0)
        G.op_cpy_indirect(k_r.reshape(1, n_k), k_view, table, 0, kv=kt if kt != "f16" else "q8_0")
        G.op_cpy_indirect(v, v_view, table, 1, kv=vt if vt != "f16" else "q8_0")
        win = lambda c, rb, t: side(t, torch, c[:w].view(w, n_head_kv, rb).permute(1, 0, 2).contiguous().view(1, n_head_kv, w, rb))
        ref = G.op_flash_attn_ext(q_r.view(1, n_head, 1, hd), win(kc2, krb, kt), win(vc2, vrb, vt), mask[:w].view(1, w), scale,
                                  kv=kt if kt != "f16" else "q8_0", kv_v=vt if vt != "f16" else None, kv_mixed=True)
        torch.cuda.synchronize()
        assert plan.status() == 0
        got = out.cpu().numpy().reshape(-1)
        assert np.isfinite(got).all(), step
        assert np.array_equal(bits(got), bits(ref.cpu().numpy().reshape(-1))), (step, np.abs(got - ref.cpu().numpy().reshape(-1)).max())
    assert windows == {64, 96}
    assert np.array_equal(kc1.cpu().numpy(), kc2.cpu().numpy()) and np.array_equal(vc1.cpu().numpy(), vc2.cpu().numpy())
    plan.close()


# ---- refusals: an error from Plan(...), nothing launched ----

def refused(G, torch, st, pattern, exc=None):
    out_before, kc_before, vc_before = st.out.clone(), st.kc.clone(), st.vc.clone()
    with pytest.raises(exc or G.Mi355qError, match=pattern) as ei:
        G.Plan(st.stages)
    assert torch.equal(st.out, out_before) and torch.equal(st.kc, kc_before) and torch.equal(st.vc, vc_before)      # nothing was launched
    return str(ei.value)


def lds_limit(G, torch, kt, vt, hd=128, E=256):
    """The pair's longest per-split window by DESIGN.md 5.6c's formula: the room the plan's fixed parts leave, over 8 + k_rb + v_rb bytes per position.
    fixed: the activation image of the E-element Q4_K GEMV stage (Q8_K in LDS: E quants, 4 bytes per 256 and per 16 elements, rounded up to 16),
    64 + 128 + 1024 bytes of control words; then 64 bytes of slack and the stage's vectors, 4 (16 + 4 hd + 72)."""
    image = (E + E // 256 * 4 + E // 16 * 4 + 15) // 16 * 16
    room = 160 * 1024 - 64 - (image + 64 + 8 * 16 + 1024) - 64 - 4 * (16 + 4 * hd + 72)
    return room // (8 + hd // 32 * BB[kt] + hd // 32 * BB[vt]) // 32 * 32


@pytest.mark.parametrize("pair", [("q8_0", "q4_0"), ("f16", "q8_0"), ("iq4_nl", "f16")], ids=ids)
def test_window_past_the_lds_limit_is_refused(G, torch, pair, monkeypatch):
    monkeypatch.setenv("MI355Q_PLAN_KV_SPLIT", "1")
    limit = lds_limit(G, torch, *pair)
    G.Plan(Stage(G, torch, pair[0], pair[1], 4, 2, 128, limit, limit - 1, "f16", seed=5).stages).close()          # the limit itself is accepted
    st = Stage(G, torch, pair[0], pair[1], 4, 2, 128, limit + 32, limit, "f16", seed=5)
    msg = refused(G, torch, st, rf"a {pair[0]} / {pair[1]} KV window of {limit + 32} positions per split \(1 split\(s\)\) does not fit the LDS: at most {limit} positions per split")
    assert str(limit) in msg


@pytest.mark.parametrize("pair", [("q8_0", "q4_0"), ("f16", "q4_1"), ("q5_0", "f16")], ids=ids)
def test_head_dim_80_is_refused(G, torch, pair):
    st = Stage(G, torch, pair[0], pair[1], 4, 4, 64, 64, 40, "f16", seed=2)
    st.attn.update(head_dim=80, q=st.q[:, :320], k=st.k[:, :320], v=st.v[:, :320], out=st.out[:, :320], rope=dict(n_dims=80))
    refused(G, torch, st, rf"a {pair[0]} / {pair[1]} KV cache needs head_dim % 32 == 0")


@pytest.mark.parametrize("pair", [("q8_0", "q4_0"), ("q8_0", "f16"), ("f16", "q8_0")], ids=ids)
def test_transposed_v_is_refused(G, torch, pair):
    st = Stage(G, torch, pair[0], pair[1], 4, 4, 64, 64, 40, "f16", seed=2)
    st.attn.update(v_nb_pos=st.attn["v_nb_dim"], v_nb_dim=st.vrow)            # the transposed layout of the non-flash graph
    refused(G, torch, st, r"flash layout.*transposed V cache is not supported")


def test_two_v_bits_are_refused(G, torch):
    st = Stage(G, torch, "q8_0", "q4_0", 4, 2, 64, 64, 40, "f16", seed=2)
    import ggml_mi355 as g
    saved = dict(g._STAGE_KVV)
    try:
        g._STAGE_KVV["q4_0"] = 0x400 | 0x1000
        refused(G, torch, st, r"more than one MI355Q_STAGE_KVV_\* flag")
    finally:
        g._STAGE_KVV.clear(); g._STAGE_KVV.update(saved)


@pytest.mark.parametrize("which", ["kv", "kv_v"])
def test_bf16_is_refused(G, torch, which):
    st = Stage(G, torch, "q8_0", "q4_0", 4, 2, 64, 64, 40, "f16", seed=2)
    st.attn[which] = "bf16"
    refused(G, torch, st, r"no attention stage for a bf16 cache side", exc=ValueError)


RING_SCRIPT = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import numpy as np, torch
import ggml_mi355 as G
from test_gpu_plan_kvmix import Stage
st = Stage(G, torch, sys.argv[4], sys.argv[5], 4, 2, 64, 64, 40, "f16", seed=4, E=256)
before = st.out.clone()
try:
    G.Plan(st.stages)
except G.Mi355qError as e:
    print("REFUSED:", e, "| untouched:", bool(torch.equal(st.out, before)))
    sys.exit(0)
print("ACCEPTED")
sys.exit(1)
"""


@pytest.mark.parametrize("pair", [("q8_0", "q4_0"), ("f16", "q8_0"), ("q8_0", "f16")], ids=ids)
def test_ring_engine_refuses_a_mixed_stage(pair):
    # (the engine is chosen once per process: a fresh interpreter)
    env = dict(os.environ, MI355Q_PLAN_ENGINE="ring")
    r = subprocess.run([sys.executable, "-c", RING_SCRIPT, str(ROOT), str(PKG), str(ROOT / "tests"), *pair], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and re.search(r"REFUSED:.*ring engine.*mixed K / V cache types.*untouched: True", r.stdout), (r.stdout[-2000:], r.stderr[-2000:])
