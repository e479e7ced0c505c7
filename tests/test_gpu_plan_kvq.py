"""The decode plan's attention stage over a Q4_1 / Q5_0 / Q5_1 / IQ4_NL KV cache (mi355q_stage.flags MI355Q_STAGE_KV_Q4_1 / _Q5_0 / _Q5_1 / _IQ4_NL;
`-fa 1 -ctk T -ctv T`), in the pattern of tests/test_gpu_plan_quant_kv.py (the Q8_0 / Q4_0 stage), regs engine.

What is compared with what:
  * the K / V blocks the stage stores for this token: byte for byte against mi355q_op_cpy of the device's own roped k / v; every other cache row is
    left as it was;
  * the output with one KV split (windows <= 256, or MI355Q_PLAN_KV_SPLIT=1): bit for bit against mi355q_op_flash_attn_ext on the same cache AND
    against tests/kvq_ref.py (pinned to the reference by tests/test_kvq_golden.py);
  * several splits (windows above 256): against the restatement within 8e-7 of max|ref|, the bound the project holds Q8_0 / Q4_0 to;
  * a 24-token decode loop against the node ops (op_rope -> op_cpy_indirect -> op_flash_attn_ext) on a twin cache: the same bits at every step;
  * refused at plan creation, nothing launched: windows beyond the type's LDS limit (the message gives the limit), head sizes that are not whole
    blocks, the transposed V layout, two cache flags at once, the ring engine.
Never-written cache blocks beyond the token hold NaN scales: a masked position must not be read.
"""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import kvq_ref
import oracle
from conftest import PKG, ROOT
from qdata import quantized_weights

pytestmark = pytest.mark.gpu

KVS = list(kvq_ref.TYPES)
BB = {kv: kvq_ref.block_bytes(kv) for kv in KVS}
# multi-split error against the CPU's single walk, as max|got - ref| / max|ref|: the bound of the Q8_0 / Q4_0 stage
SPLIT_BOUND = 8e-7


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


def quantize_rows(G, torch, x, kv):
    """op_cpy f32 [n, m] -> uint8 [n, m / 32 * BB] on the device."""
    out = torch.zeros((x.shape[0], x.shape[1] // 32 * BB[kv]), dtype=torch.uint8, device="cuda")
    G.op_cpy(x, out, kv=kv)
    return out


def poison(cache_np, rows, kv):
    """NaN block scales in the given rows (never-written cache cells)."""
    c = cache_np.copy()
    nb = c.shape[1] // BB[kv]
    blocks = c.reshape(c.shape[0], nb, BB[kv])
    blocks[rows, :, 0:2] = np.array([0x00, 0x7E], np.uint8)          # f16 NaN, little endian
    return c


class Stage:
    """A GEMV stage producing q / k / v, then the quantized-cache attention stage, on random inputs."""

    def __init__(self, G, torch, kv, n_head, n_head_kv, hd, n_kv, pos, mask_kind="f16", mode=0, seed=0, E=256):
        rng = np.random.default_rng(seed)
        self.G, self.torch, self.kv = G, torch, kv
        self.n_head, self.n_head_kv, self.hd, self.n_kv, self.pos, self.mode = n_head, n_head_kv, hd, n_kv, pos, mode
        n_q, n_k = n_head * hd, n_head_kv * hd
        self.rb = hd // 32 * BB[kv]
        self.row = n_head_kv * self.rb                                    # bytes per cache position
        n_ctx = n_kv + 32
        wq, wk, wv = W(G, oracle.Q4_K, n_q, E, rng), W(G, oracle.Q4_K, n_k, E, rng), W(G, oracle.Q4_K, n_k, E, rng)
        x = dev(torch, rng.standard_normal((1, E)).astype(np.float32))
        self.q, self.k, self.v = (torch.zeros((1, n), dtype=torch.float32, device="cuda") for n in (n_q, n_k, n_k))
        self.out = torch.zeros((1, n_q), dtype=torch.float32, device="cuda")
        kc = quantize_rows(G, torch, dev(torch, rng.standard_normal((n_ctx, n_k)).astype(np.float32)), kv).cpu().numpy()
        vc = quantize_rows(G, torch, dev(torch, rng.standard_normal((n_ctx, n_k)).astype(np.float32)), kv).cpu().numpy()
        self.kc_h, self.vc_h = poison(kc, slice(pos + 1, None), kv), poison(vc, slice(pos + 1, None), kv)
        self.kc, self.vc = dev(torch, self.kc_h), dev(torch, self.vc_h)
        if mask_kind is None:
            assert n_kv == pos + 1                                        # (no mask: the window is exactly the written positions)
            self.mask_h = None; mask = None
        else:
            self.mask_h = np.full(n_kv, -np.inf, np.float32)
            self.mask_h[:pos + 1] = rng.choice(np.array([0.0, 0.0, -0.5, -1.25], np.float32), pos + 1)   # (values exact in f16)
            mask = dev(torch, self.mask_h if mask_kind == "f32" else self.mask_h.astype(np.float16))
        self.posd = dev(torch, np.array([pos], np.int32))
        self.dst = torch.tensor([self.kc.data_ptr() + pos * self.row, self.vc.data_ptr() + pos * self.row], dtype=torch.int64, device="cuda")
        self.scale = 1.0 / np.sqrt(hd)
        self.attn = dict(q=self.q, k=self.k, v=self.v, pos=self.posd, rope=dict(n_dims=hd, mode=mode, n_ctx_orig=8192, freq_base=500000.0),
                         k_cache=self.kc, v_cache=self.vc, k_nb_pos=self.row, k_nb_head=self.rb, v_nb_pos=self.row, v_nb_dim=BB[kv], v_nb_head=self.rb,
                         k_dst=self.dst[0:1], v_dst=self.dst[1:2], v_dst_nb=0, mask=mask, n_head=n_head, n_head_kv=n_head_kv, head_dim=hd, n_kv=n_kv,
                         scale=self.scale, out=self.out, kv=kv)
        self.stages = [dict(ws=[wq, wk, wv], ys=[self.q, self.k, self.v], x=x), dict(attn=self.attn)]

    def run(self):
        plan = self.G.Plan(self.stages)
        plan.run(); self.torch.cuda.synchronize()
        assert plan.status() == 0
        plan.close()

    def rope(self, t, n):
        return self.G.op_rope(t.view(1, 1, n, self.hd), self.posd, self.hd, self.mode, n_ctx_orig=8192, freq_base=500000.0)

    def check_stores(self):
        """The stored rows are op_cpy of the device's roped k / v; nothing else changed.  Returns the caches as they now are."""
        torch, n_k = self.torch, self.n_head_kv * self.hd
        k_r = self.rope(self.k, self.n_head_kv).reshape(1, n_k)
        want_k = quantize_rows(self.G, torch, k_r, self.kv).cpu().numpy()[0]
        want_v = quantize_rows(self.G, torch, self.v, self.kv).cpu().numpy()[0]
        kc, vc = self.kc.cpu().numpy(), self.vc.cpu().numpy()
        assert np.array_equal(kc[self.pos], want_k) and np.array_equal(vc[self.pos], want_v)
        other = np.ones(kc.shape[0], bool); other[self.pos] = False
        assert np.array_equal(kc[other], self.kc_h[other]) and np.array_equal(vc[other], self.vc_h[other])
        return kc, vc

    def reference(self, kc, vc):
        """kvq_ref.flash_attn_ext on the device's roped q and the cache as stored -> [n_head, hd] f32."""
        q_r = self.rope(self.q, self.n_head).cpu().numpy().reshape(1, self.n_head, 1, self.hd)
        win = lambda c: c[:self.n_kv].reshape(self.n_kv, self.n_head_kv, self.rb).transpose(1, 0, 2)[None]
        mask = None if self.mask_h is None else self.mask_h.reshape(1, self.n_kv)
        return kvq_ref.flash_attn_ext(self.kv, q_r, win(kc), win(vc), mask, self.scale).reshape(self.n_head, self.hd)

    def node_op(self, kc, vc):
        """mi355q_op_flash_attn_ext on the device's roped q and the same cache -> [n_head, hd] f32."""
        G, torch = self.G, self.torch
        q_r = self.rope(self.q, self.n_head).view(1, self.n_head, 1, self.hd)
        win = lambda c: dev(torch, c[:self.n_kv].reshape(self.n_kv, self.n_head_kv, self.rb).transpose(1, 0, 2)[None])
        mask = None if self.mask_h is None else dev(torch, self.mask_h.astype(np.float16).reshape(1, self.n_kv))
        return G.op_flash_attn_ext(q_r, win(kc), win(vc), mask, float(self.scale), kv=self.kv).cpu().numpy().reshape(self.n_head, self.hd)

    def got(self):
        return self.out.cpu().numpy().reshape(self.n_head, self.hd)


SHAPES = {"32-8-128": (32, 8, 128, 256, 200, 0), "4-2-64-neox": (4, 2, 64, 64, 40, 2), "8-8-96": (8, 8, 96, 128, 100, 0)}


@pytest.mark.parametrize("mask", ["f16", "f32", None], ids=["mask_f16", "mask_f32", "no_mask"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize("kv", KVS)
def test_one_split_is_the_cpu_bits(G, torch, kv, shape, mask):
    n_head, n_head_kv, hd, n_kv, pos, mode = SHAPES[shape]
    if mask is None:
        n_kv = pos + 1
    st = Stage(G, torch, kv, n_head, n_head_kv, hd, n_kv, pos, mask, mode, seed=zlib.crc32(f"{kv}{shape}{mask}".encode()) % 1000)
    st.run()
    kc, vc = st.check_stores()
    got, ref = st.got(), st.reference(kc, vc)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.abs(got - ref).max()
    assert np.array_equal(got.view(np.uint32), st.node_op(kc, vc).view(np.uint32))


@pytest.mark.parametrize("kv", KVS)
def test_forced_single_split_is_the_cpu_bits(G, torch, kv, monkeypatch):
    monkeypatch.setenv("MI355Q_PLAN_KV_SPLIT", "1")
    st = Stage(G, torch, kv, 32, 8, 128, 512, 450, "f16", seed=3)
    st.run()
    kc, vc = st.check_stores()
    got, ref = st.got(), st.reference(kc, vc)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.abs(got - ref).max()


def _plan_accepts(G, torch, kv, n_kv):
    st = Stage(G, torch, kv, 32, 8, 128, n_kv, n_kv - 1, "f16", seed=5, E=256)
    try:
        G.Plan(st.stages).close()
        return True
    except G.Mi355qError as e:
        assert "does not fit the LDS" in str(e), str(e)
        return False


@pytest.fixture(scope="module")
def largest(G, torch):
    """The largest window (a multiple of 32) a Llama-3-8B-shaped stage accepts, per cache type: searched through plan_create."""
    out = {}
    for kv in KVS:
        lo, hi = 2048, 16384
        assert _plan_accepts(G, torch, kv, lo)
        while hi - lo > 32:
            mid = (lo + hi) // 2 // 32 * 32
            lo, hi = (mid, hi) if _plan_accepts(G, torch, kv, mid) else (lo, mid)
        out[kv] = lo
    print("largest accepted windows (32 heads, 8 splits):", out)
    return out


@pytest.mark.parametrize("n_kv", [512, 2048, "largest"])
@pytest.mark.parametrize("kv", KVS)
def test_several_splits_within_the_bound(G, torch, kv, n_kv, largest):
    n_kv = largest[kv] if n_kv == "largest" else n_kv
    st = Stage(G, torch, kv, 32, 8, 128, n_kv, n_kv - 7, "f16", seed=n_kv % 97)
    st.run()
    kc, vc = st.check_stores()
    got, ref = st.got(), st.reference(kc, vc)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"{kv} n_kv {n_kv}: max error {err:.3e} of max|out|")
    assert err <= SPLIT_BOUND, err


def test_limits(G, torch, largest):
    """Each type has its own longest window: the LDS formula of DESIGN.md 5.6c with the type's block bytes (smaller blocks, longer windows)."""
    fixed = None
    for kv in KVS:
        st = Stage(G, torch, kv, 32, 8, 128, largest[kv] + 64, largest[kv], "f16", seed=1, E=256)
        out_before = st.out.clone()
        with pytest.raises(G.Mi355qError, match="does not fit the LDS") as ei:
            G.Plan(st.stages)
        m = re.search(rf"a {kv} KV window of (\d+) positions per split \((\d+) split\(s\)\) does not fit the LDS: at most (\d+) positions per split", str(ei.value))
        assert m, str(ei.value)
        per, n_split, limit = map(int, m.groups())
        assert per > limit and limit % 32 == 0 and limit * n_split >= largest[kv] > (limit - 32) * n_split, (kv, per, n_split, limit, largest[kv])
        assert torch.equal(st.out, out_before)                               # nothing was launched
        # limit = floor32((room) / (8 + 2 * rb)): the same room for every type
        room_lo, room_hi = limit * (8 + 2 * st.rb), (limit + 32) * (8 + 2 * st.rb)
        fixed = (room_lo, room_hi) if fixed is None else (max(fixed[0], room_lo), min(fixed[1], room_hi))
        assert fixed[0] < fixed[1], (kv, fixed)
    assert largest["q4_1"] >= 8 * 320                                        # Llama-3-8B's shape reaches at least what the f16 LDS form reaches
    assert largest["iq4_nl"] >= largest["q4_1"] >= largest["q5_0"] >= largest["q5_1"]


def test_two_cache_flags_are_refused(G, torch):
    st = Stage(G, torch, "q4_1", 4, 2, 64, 64, 40, "f16", seed=2, E=256)
    import ggml_mi355 as g
    saved = dict(g._STAGE_KV)
    try:
        g._STAGE_KV["q4_1"] = 0x10 | 0x40
        with pytest.raises(G.Mi355qError, match="more than one"):
            G.Plan(st.stages)
    finally:
        g._STAGE_KV.clear(); g._STAGE_KV.update(saved)


@pytest.mark.parametrize("kv", KVS)
def test_partial_blocks_and_transposed_v_are_refused(G, torch, kv):
    st = Stage(G, torch, kv, 4, 4, 64, 64, 40, "f16", seed=2, E=256)
    st.attn.update(head_dim=80, q=st.q[:, :320], k=st.k[:, :320], v=st.v[:, :320], out=st.out[:, :320], rope=dict(n_dims=80), k_nb_head=80 // 32 * BB[kv])
    with pytest.raises(G.Mi355qError):
        G.Plan(st.stages)
    st = Stage(G, torch, kv, 4, 4, 64, 64, 40, "f16", seed=2, E=256)
    st.attn.update(v_nb_pos=BB[kv], v_nb_dim=st.row)                    # the transposed layout of the non-flash graph
    with pytest.raises(G.Mi355qError, match="flash layout"):
        G.Plan(st.stages)


@pytest.mark.parametrize("kv", KVS)
def test_decode_loop_matches_the_node_ops(G, torch, kv):
    """24 tokens through ONE plan whose K / V destinations move every token, against op_rope -> op_cpy_indirect -> op_flash_attn_ext on a twin cache."""
    n_head, n_head_kv, hd, n_kv, p0 = 32, 8, 128, 96, 50
    rng = np.random.default_rng(11)
    n_q, n_k = n_head * hd, n_head_kv * hd
    rb = hd // 32 * BB[kv]; row = n_head_kv * rb
    q, k, v = (torch.zeros((1, n), dtype=torch.float32, device="cuda") for n in (n_q, n_k, n_k))
    out = torch.zeros((1, n_q), dtype=torch.float32, device="cuda")
    init = [quantize_rows(G, torch, dev(torch, rng.standard_normal((n_kv, n_k)).astype(np.float32)), kv).cpu().numpy() for _ in range(2)]
    kc1, vc1 = (dev(torch, poison(c, slice(p0, None), kv)) for c in init)          # plan
    kc2, vc2 = kc1.clone(), vc1.clone()                                           # node ops
    mask_h = np.full(n_kv, -np.inf, np.float16)
    mask = dev(torch, mask_h)
    posd = dev(torch, np.array([p0], np.int32))
    dst = torch.tensor([kc1.data_ptr() + p0 * row, vc1.data_ptr() + p0 * row], dtype=torch.int64, device="cuda")
    table = torch.tensor([kc2.data_ptr() + p0 * row, vc2.data_ptr() + p0 * row], dtype=torch.int64, device="cuda")
    scale = 1.0 / np.sqrt(hd)
    w0 = W(G, oracle.Q4_K, 32, 256, rng); x0 = torch.zeros((1, 256), dtype=torch.float32, device="cuda"); y0 = torch.zeros((1, 32), dtype=torch.float32, device="cuda")
    attn = dict(q=q, k=k, v=v, pos=posd, rope=dict(n_dims=hd, mode=0, n_ctx_orig=8192, freq_base=500000.0), k_cache=kc1, v_cache=vc1,
                k_nb_pos=row, k_nb_head=rb, v_nb_pos=row, v_nb_dim=BB[kv], v_nb_head=rb, k_dst=dst[0:1], v_dst=dst[1:2], v_dst_nb=0,
                mask=mask, n_head=n_head, n_head_kv=n_head_kv, head_dim=hd, n_kv=n_kv, scale=scale, out=out, kv=kv)
    plan = G.Plan([([w0], x0, [y0], False), dict(attn=attn)])
    row_view = torch.zeros((1, row), dtype=torch.uint8, device="cuda")           # (type and shape of the indirect stores; data from the table)
    for step in range(24):
        p = p0 + step
        for t in (q, k, v):
            t.copy_(dev(torch, rng.standard_normal(t.shape).astype(np.float32)))
        posd.fill_(p)
        mask_h[:p + 1] = 0.0
        mask.copy_(dev(torch, mask_h))
        dst.copy_(torch.tensor([kc1.data_ptr() + p * row, vc1.data_ptr() + p * row], dtype=torch.int64))
        table.copy_(torch.tensor([kc2.data_ptr() + p * row, vc2.data_ptr() + p * row], dtype=torch.int64))
        plan.run()
        q_r = G.op_rope(q.view(1, 1, n_head, hd), posd, hd, 0, n_ctx_orig=8192, freq_base=500000.0)
        k_r = G.op_rope(k.view(1, 1, n_head_kv, hd), posd, hd, 0, n_ctx_orig=8192, freq_base=500000.0)
        G.op_cpy_indirect(k_r.reshape(1, n_k), row_view, table, 0, kv=kv)
        G.op_cpy_indirect(v, row_view, table, 1, kv=kv)
        win = lambda c: c.view(n_kv, n_head_kv, rb).permute(1, 0, 2).contiguous().view(1, n_head_kv, n_kv, rb)
        ref = G.op_flash_attn_ext(q_r.view(1, n_head, 1, hd), win(kc2), win(vc2), mask.view(1, n_kv), scale, kv=kv)
        torch.cuda.synchronize()
        assert plan.status() == 0
        got = out.cpu().numpy().reshape(-1)
        assert np.isfinite(got).all(), step
        assert np.array_equal(got.view(np.uint32), ref.cpu().numpy().reshape(-1).view(np.uint32)), (step, np.abs(got - ref.cpu().numpy().reshape(-1)).max())
    assert np.array_equal(kc1.cpu().numpy(), kc2.cpu().numpy()) and np.array_equal(vc1.cpu().numpy(), vc2.cpu().numpy())
    plan.close()


RING_SCRIPT = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import numpy as np, torch
import ggml_mi355 as G
from test_gpu_plan_kvq import Stage
st = Stage(G, torch, sys.argv[4], 4, 2, 64, 64, 40, "f16", seed=4, E=256)
try:
    G.Plan(st.stages)
except G.Mi355qError as e:
    print("REFUSED:", e)
    sys.exit(0)
print("ACCEPTED")
sys.exit(1)
"""


@pytest.mark.parametrize("kv", KVS)
def test_ring_engine_refuses_a_quantized_stage(kv):
    # (the engine is chosen once per process: a fresh interpreter)
    env = dict(os.environ, MI355Q_PLAN_ENGINE="ring")
    r = subprocess.run([sys.executable, "-c", RING_SCRIPT, str(ROOT), str(PKG), str(ROOT / "tests"), kv], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REFUSED" in r.stdout and "ring" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
