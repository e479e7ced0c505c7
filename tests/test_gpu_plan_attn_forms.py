"""Every form of the decode plan's attention stage (csrc/plan.hip), reached on purpose and checked against a plain reference.

mi355q_plan_create picks one kernel per attention stage ("Attention forms"):
  fa_seq     plan_attn_lds, flash layout (V rows per position), one KV split: the CPU's sequential F16 accumulator
  p_f16      plan_attn_lds, transposed V, one split: the CPU's f16-rounded probabilities
  lds        plan_attn_lds with f32 accumulation: several splits (merged by COMBINE), or the flash layout with MI355Q_PLAN_FA_EXACT=0
  global     plan_attn from global memory: the window does not fit the LDS, per > 320, an unaligned cache or MI355Q_PLAN_KV_LDS=0
  fallback   plan_attn chosen at RUN time by plan_attn_lds: a transposed V window whose per-split length or n_kv is not a multiple of 8
Each test asserts the form through the MI355Q_PLAN_VERBOSE line of plan_create ("window in / not in LDS", the split count, "sequential f16
accumulation"); the run-time fallback prints nothing, so its cases assert the create-time line and the arithmetic that sends them there.

What is compared with what:
  * the K / V rows the stage stores: bit for bit against mi355q_op_rope then mi355q_op_cpy on the device's own k / v (both pinned to the CPU in
    tests/test_gpu_glue.py), with the same rope options; every other cache row keeps its bits;
  * f32 forms: a float64 restatement (q roped by mi355q_op_rope -- the stage's own rotation, checked against oracle/glue.py rope to 1e-5 --
    and rounded to f16; softmax(q.k scale + mask) V over the live positions);
  * p_f16 (one split, transposed V): the same with the CPU's probabilities (f32 exponentials, f64 sum, rounded to f16);
  * fa_seq: oracle/glue.py flash_attn_ext, bit for bit;
  * masked and out-of-window cache rows are filled once with NaN and once with +-65504 (K) / +-Inf (V): both must pass, and give the same bits.
The mask entries beyond the run's window are 0 (they are not part of the window: a stage that reads them would take garbage rows as live).
"""
import os
import re
import zlib
from contextlib import contextmanager

import numpy as np
import pytest

import oracle
from oracle import glue
from qdata import quantized_weights

pytestmark = pytest.mark.gpu

# Bounds as max|got - ref| / max|ref|, about four times the largest error measured on an MI355X over this file's cases (and the ring engine's):
# f32 forms against float64: f32 summation order only (measured at most 4.0e-6; test_gpu_plan.py test_attention_stage uses the same bound)
F32_BOUND = 2e-5
# f16-rounded probabilities: a device expf one ulp from numpy's can flip a probability's rounding, 2^-11 of it (measured at most 2.1e-5)
P_F16_BOUND = 1e-4

VERBOSE = re.compile(r"attention stage \d+: n_kv (\d+), (\d+) split\(s\) of (\d+) positions, window (in|not in) LDS(, sequential f16 accumulation)?")


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


@contextmanager
def env(**kw):
    """Set (None: unset) environment variables for the duration (plan_create reads MI355Q_PLAN_* when it runs)."""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# the variables that steer plan_create's choice of form: unset unless a case sets them (a value left in the environment would change every form)
FORM_ENV = dict(MI355Q_PLAN_KV_SPLIT=None, MI355Q_PLAN_KV_LDS=None, MI355Q_PLAN_FA_EXACT=None)


def n_cu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected_splits(torch, n_head, n_kv):
    """plan_create's KV split count: one per 256 positions, at most #CU / n_head."""
    return max(1, min((n_kv + 255) // 256, n_cu(torch) // n_head))


def seed_of(*a):
    return zlib.crc32(repr(a).encode()) % 100000


def fill_garbage(rows_k, rows_v, garbage):
    """Never-written cache rows: NaN, or +-65504 in K and +-Inf in V (alternating by element)."""
    if garbage == "nan":
        rows_k[...] = np.float16(np.nan); rows_v[...] = np.float16(np.nan)
    else:
        sgn = np.where(np.arange(rows_k.shape[-1]) % 2 == 0, 1.0, -1.0)
        rows_k[...] = (sgn * 65504.0).astype(np.float16); rows_v[...] = (sgn * np.inf).astype(np.float16)


class Case:
    """A GEMV stage producing q / k / v from a random vector, then the f16-cache attention stage.

    slot: the cache cell this token's K / V row goes to (window position slot); pos: the rope position (default slot);
    live: bool [n_kv] -- the window positions the mask leaves open (default: 0 ..= slot); mask: "f32", "f16" or None (no mask: every position of
    the run's window is live); n_kv_dev: the per-run window (None: n_kv); k_off: bytes added to both cache base addresses."""

    def __init__(self, G, torch, n_head, n_head_kv, hd, n_kv, slot, layout="rows_v", mask="f32", live=None, pos=None, rope=None, ff=None,
                 n_kv_dev=None, k_off=0, seed=0, E=256):
        rng = np.random.default_rng(seed)
        self.G, self.torch = G, torch
        self.n_head, self.n_head_kv, self.hd, self.n_kv, self.slot, self.layout = n_head, n_head_kv, hd, n_kv, slot, layout
        self.pos = slot if pos is None else pos
        self.rp = dict(n_dims=hd, mode=0, n_ctx_orig=8192, freq_base=500000.0, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0)
        self.rp.update(rope or {})
        self.ff = None if ff is None else np.asarray(ff, np.float32)
        n_q, n_k = n_head * hd, n_head_kv * hd
        self.n_q, self.n_k = n_q, n_k
        self.w = n_kv if n_kv_dev is None else min(n_kv, max(1, n_kv_dev))          # the run's window
        assert 0 <= slot < self.w
        self.n_ctx = n_ctx = (max(n_kv, slot + 1) + 32 + 31) // 32 * 32
        wq, wk, wv = (G.QWeight.from_host(oracle.Q4_K, quantized_weights(oracle.Q4_K, m, E, rng), m, E) for m in (n_q, n_k, n_k))
        x = torch.from_numpy(rng.standard_normal((1, E)).astype(np.float32)).cuda()
        self.q, self.k, self.v = (torch.zeros((1, n), dtype=torch.float32, device="cuda") for n in (n_q, n_k, n_k))
        self.out = torch.zeros((1, n_q), dtype=torch.float32, device="cuda")
        if mask is None:
            self.live = np.ones(n_kv, bool)
            self.mask_h = None
        else:
            self.live = np.zeros(n_kv, bool)
            if live is None:
                self.live[:slot + 1] = True
            else:
                self.live[:] = live
        self.live[self.w:] = False
        assert self.live[slot]
        if mask is not None:
            self.mask_h = np.zeros(n_ctx, np.float32)                                # beyond the run's window: 0 (not part of the window)
            self.mask_h[:self.w] = -np.inf
            live_idx = np.flatnonzero(self.live)
            self.mask_h[live_idx] = rng.choice(np.array([0.0, 0.0, -0.5, -1.25], np.float32), live_idx.size)   # (exact in f16)
        self.kc_fin = rng.standard_normal((n_ctx, n_k)).astype(np.float16)           # [position][kv head * hd], logical for both layouts
        self.vc_fin = rng.standard_normal((n_ctx, n_k)).astype(np.float16)
        assert k_off % 2 == 0
        eo = k_off // 2
        self.kbuf = torch.zeros(n_ctx * n_k + eo, dtype=torch.float16, device="cuda")
        self.vbuf = torch.zeros(n_ctx * n_k + eo, dtype=torch.float16, device="cuda")
        self.kc = self.kbuf[eo:].view(n_ctx, n_k)
        self.vc = self.vbuf[eo:].view(n_ctx, n_k) if layout == "rows_v" else self.vbuf[eo:].view(n_k, n_ctx)
        if layout == "rows_v":
            vl = dict(v_nb_pos=n_k * 2, v_nb_dim=2, v_nb_head=hd * 2, v_dst_nb=2)
            v_dst = self.vc.data_ptr() + slot * n_k * 2
        else:
            vl = dict(v_nb_pos=2, v_nb_dim=n_ctx * 2, v_nb_head=hd * n_ctx * 2, v_dst_nb=n_ctx * 2)
            v_dst = self.vc.data_ptr() + slot * 2
        self.posd = torch.tensor([self.pos], dtype=torch.int32, device="cuda")
        self.dst = torch.tensor([self.kc.data_ptr() + slot * n_k * 2, v_dst], dtype=torch.int64, device="cuda")
        self.ffd = None if self.ff is None else torch.from_numpy(self.ff).cuda()
        self.nkvd = None if n_kv_dev is None else torch.tensor([n_kv_dev], dtype=torch.int32, device="cuda")
        self.maskd = None
        if mask is not None:
            m = self.mask_h if mask == "f32" else self.mask_h.astype(np.float16)
            self.maskd = torch.from_numpy(m).cuda()
        self.scale = 1.0 / np.sqrt(hd)
        rope_arg = {k_: self.rp[k_] for k_ in ("n_dims", "mode", "n_ctx_orig", "freq_base", "freq_scale", "ext_factor", "attn_factor", "beta_fast", "beta_slow")}
        self.attn = dict(q=self.q, k=self.k, v=self.v, pos=self.posd, n_kv_dev=self.nkvd, rope=rope_arg, freq_factors=self.ffd,
                         k_cache=self.kc, v_cache=self.vc, k_nb_pos=n_k * 2, k_nb_head=hd * 2, k_dst=self.dst[0:1], v_dst=self.dst[1:2], mask=self.maskd,
                         n_head=n_head, n_head_kv=n_head_kv, head_dim=hd, n_kv=n_kv, scale=self.scale, out=self.out, **vl)
        self.stages = [dict(ws=[wq, wk, wv], ys=[self.q, self.k, self.v], x=x), dict(attn=self.attn)]
        self.plan = None

    # ---- running ----
    def create(self, **envs):
        with env(**dict(FORM_ENV, **envs)):
            self.plan = self.G.Plan(self.stages)
        return self.plan

    def load(self, garbage):
        """Upload the caches: live positions finite, every other row (masked, beyond the window, this token's own cell) garbage."""
        kc, vc = self.kc_fin.copy(), self.vc_fin.copy()
        dead = np.ones(self.n_ctx, bool); dead[:self.n_kv] = ~self.live; dead[self.slot] = True
        kg, vg = kc[dead], vc[dead]                                                  # (fancy indexing copies: fill, then write back)
        fill_garbage(kg, vg, garbage)
        kc[dead], vc[dead] = kg, vg
        self.kc_h, self.vc_h = kc, vc
        self.kc.copy_(self.torch.from_numpy(kc))
        self.vc.copy_(self.torch.from_numpy(vc if self.layout == "rows_v" else np.ascontiguousarray(vc.T)))

    def run(self, garbage="nan"):
        if self.plan is None:
            self.create()
        self.load(garbage)
        self.out.fill_(12345.0)
        self.plan.run(); self.torch.cuda.synchronize()
        assert self.plan.status() == 0

    def close(self):
        if self.plan is not None:
            self.plan.close(); self.plan = None

    # ---- checking ----
    def caches(self):
        kc = self.kc.cpu().numpy()
        vc = self.vc.cpu().numpy()
        return kc, (vc if self.layout == "rows_v" else np.ascontiguousarray(vc.T))

    def rope_dev(self, t, n):
        r = self.rp
        return self.G.op_rope(t.view(1, 1, n, self.hd), self.posd, r["n_dims"], r["mode"], freq_factors=self.ffd, n_ctx_orig=r["n_ctx_orig"],
                              freq_base=r["freq_base"], freq_scale=r["freq_scale"], ext_factor=r["ext_factor"], attn_factor=r["attn_factor"],
                              beta_fast=r["beta_fast"], beta_slow=r["beta_slow"])

    def check_stores(self):
        """This token's rows are op_cpy(op_rope(k)) and op_cpy(v), bit for bit; every other row keeps its bits.  Returns the caches."""
        torch = self.torch
        want_k = torch.zeros((1, self.n_k), dtype=torch.float16, device="cuda"); want_v = torch.zeros((1, self.n_k), dtype=torch.float16, device="cuda")
        self.G.op_cpy(self.rope_dev(self.k, self.n_head_kv).reshape(1, self.n_k), want_k)
        self.G.op_cpy(self.v, want_v)
        kc, vc = self.caches()
        u = lambda a: a.view(np.uint16)
        assert np.array_equal(u(kc[self.slot]), u(want_k.cpu().numpy()[0])), "stored K row"
        assert np.array_equal(u(vc[self.slot]), u(want_v.cpu().numpy()[0])), "stored V row"
        other = np.ones(self.n_ctx, bool); other[self.slot] = False
        assert np.array_equal(u(kc[other]), u(self.kc_h[other])) and np.array_equal(u(vc[other]), u(self.vc_h[other])), "other cache rows changed"
        return kc, vc

    def q_roped(self):
        """q roped by mi355q_op_rope -- the stage's own rotation, as the stored K row shows bit for bit -- after a check against oracle/glue.py
        rope (the two may differ by a cosf / sinf ulp, which can flip an f16 rounding of q and move a peaked softmax by more than F32_BOUND)."""
        r = self.rp
        qh = self.q.cpu().numpy().reshape(1, 1, self.n_head, self.hd)
        want = glue.rope(qh, np.array([self.pos], np.int32), r["n_dims"], r["mode"], self.ff, r["n_ctx_orig"], r["freq_base"], r["freq_scale"],
                         r["ext_factor"], r["attn_factor"], r["beta_fast"], r["beta_slow"]).reshape(self.n_head, self.hd)
        got = self.rope_dev(self.q, self.n_head).cpu().numpy().reshape(self.n_head, self.hd)
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
        return got

    def reference(self, kc, vc, kind):
        """kind "f32": float64 softmax; "p_f16": the CPU's f16-rounded probabilities; "fa_seq": glue.flash_attn_ext.  -> [n_head, hd] float64."""
        q_r = self.q_roped()
        idx = np.flatnonzero(self.live)
        madd = np.zeros(self.n_kv) if self.mask_h is None else self.mask_h[:self.n_kv].astype(np.float64)
        hd, gq = self.hd, self.n_head // self.n_head_kv
        if kind == "fa_seq":
            w = self.w
            K = np.where(self.live[:w, None], kc[:w], np.float16(0)); V = np.where(self.live[:w, None], vc[:w], np.float16(0))
            m = None if self.mask_h is None else self.mask_h[:w].astype(np.float16).reshape(1, w)
            o = glue.flash_attn_ext(q_r.reshape(1, self.n_head, 1, hd), K.reshape(1, w, self.n_head_kv, hd).transpose(0, 2, 1, 3),
                                    V.reshape(1, w, self.n_head_kv, hd).transpose(0, 2, 1, 3), m, self.scale)
            return o.reshape(self.n_head, hd).astype(np.float64)
        q16 = q_r.astype(np.float16).astype(np.float64)
        ref = np.zeros((self.n_head, hd))
        for h in range(self.n_head):
            g = h // gq
            Kg = kc[idx, g * hd:(g + 1) * hd].astype(np.float64); Vg = vc[idx, g * hd:(g + 1) * hd].astype(np.float64)
            s = (Kg @ q16[h]) * self.scale + madd[idx]
            if kind == "p_f16":
                s32 = s.astype(np.float32)
                e = np.exp(s32 - s32.max()).astype(np.float32)
                p = (e * np.float32(1.0 / e.astype(np.float64).sum())).astype(np.float16).astype(np.float64)
            else:
                p = np.exp(s - s.max()); p /= p.sum()
            ref[h] = p @ Vg
        return ref

    def got(self):
        return self.out.cpu().numpy().reshape(self.n_head, self.hd).astype(np.float64)


def compare(got, ref, kind, what=""):
    assert np.isfinite(got).all(), (what, "non-finite output")
    top = np.abs(ref).max()
    d = np.abs(got - ref)
    if kind == "fa_seq":
        # with q roped by the device (see Case.q_roped) the whole chain is the CPU's: measured bit-exact in every case on an MI355X
        assert np.array_equal(got.astype(np.float32).view(np.uint32), ref.astype(np.float32).view(np.uint32)), (what, d.max() / top, (d > 0).mean())
        return 0.0
    bound = P_F16_BOUND if kind == "p_f16" else F32_BOUND
    assert d.max() <= bound * top, (what, kind, d.max() / top)
    return d.max() / top


def ref_kind(case, form):
    """The reference a form is held to.  The ring engine runs every case in its global form: p_f16 at one split with a transposed V, else f32."""
    if form == "fa_seq" and os.environ.get("MI355Q_PLAN_ENGINE") != "ring":
        return "fa_seq"
    if case.layout == "transposed_v" and expected_splits(case.torch, case.n_head, case.n_kv) == 1:
        return "p_f16"
    return "f32"


def run_and_check(case, form, what=""):
    """Run with NaN garbage, check stores and output; run again with +-65504 / Inf garbage: the same bits.  Returns the relative error."""
    case.run("nan")
    kc, vc = case.check_stores()
    got = case.got()
    err = compare(got, case.reference(kc, vc, ref_kind(case, form)), ref_kind(case, form), what)
    print(f"measured: {what}: {ref_kind(case, form)} error {err:.3e} of max|out|")
    case.run("big")
    case.check_stores()
    assert np.array_equal(case.got().astype(np.float32).view(np.uint32), got.astype(np.float32).view(np.uint32)), (what, "garbage changed the output")
    return err


def parse_forms(text):
    """The verbose lines of plan_create: [(n_kv, splits, per, in_lds, seq)]."""
    return [(int(m[1]), int(m[2]), int(m[3]), m[4] == "in", m[5] is not None) for m in VERBOSE.finditer(text)]


def assert_form(text, form, splits, case):
    lines = parse_forms(text)
    assert len(lines) == 1, text
    n_kv, sp, per, in_lds, seq = lines[0]
    assert n_kv == case.n_kv and sp == splits, (lines, splits)
    if form == "fa_seq":
        assert in_lds and seq and sp == 1, lines
    elif form == "p_f16":
        assert in_lds and not seq and sp == 1 and case.layout == "transposed_v", lines
    elif form == "lds":
        assert in_lds and not seq, lines
    elif form == "global":
        assert not in_lds, lines
    elif form == "fallback":
        # plan_attn_lds hands a transposed window whose run-time per or n_kv is not a multiple of 8 to plan_attn (plan.hip, entry of plan_attn_lds)
        run_per = (case.w + sp - 1) // sp
        assert in_lds and not seq and case.layout == "transposed_v" and ((run_per | case.w) & 7) != 0, lines
    else:
        raise AssertionError(form)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# form matrix: id -> (n_head, n_head_kv, hd, n_kv, slot, layout, form, env, extra)
T, R = "transposed_v", "rows_v"
FORM_CASES = {
    # fa_seq: flash layout, one split, window in LDS -- head_dim 32 .. 256, GQA 1 / 4 / 8, MQA
    "fa_seq-8.8.32-kv128": (8, 8, 32, 128, 100, R, "fa_seq", {}, {}),
    "fa_seq-8.2.64-kv256-neox": (8, 2, 64, 256, 200, R, "fa_seq", {}, dict(rope=dict(mode=2))),
    "fa_seq-4.4.96-kv96": (4, 4, 96, 96, 50, R, "fa_seq", {}, {}),
    "fa_seq-32.8.128-kv256": (32, 8, 128, 256, 201, R, "fa_seq", {}, {}),
    "fa_seq-16.2.128-kv128-gqa8": (16, 2, 128, 128, 77, R, "fa_seq", {}, {}),
    "fa_seq-4.1.192-kv160-mqa": (4, 1, 192, 160, 150, R, "fa_seq", {}, {}),
    "fa_seq-4.4.256-kv64": (4, 4, 256, 64, 40, R, "fa_seq", {}, {}),
    # lds f32, one split: MI355Q_PLAN_FA_EXACT=0
    "lds-fa_exact0-32.8.128-kv256": (32, 8, 128, 256, 201, R, "lds", dict(MI355Q_PLAN_FA_EXACT=0), {}),
    # p_f16: transposed V, one split, window in LDS
    "p_f16-8.8.32-kv128": (8, 8, 32, 128, 100, T, "p_f16", {}, {}),
    "p_f16-8.2.64-kv256-neox": (8, 2, 64, 256, 200, T, "p_f16", {}, dict(rope=dict(mode=2))),
    "p_f16-4.4.96-kv96": (4, 4, 96, 96, 50, T, "p_f16", {}, {}),
    "p_f16-32.8.128-kv256": (32, 8, 128, 256, 201, T, "p_f16", {}, {}),
    "p_f16-4.1.192-kv160-mqa": (4, 1, 192, 160, 150, T, "p_f16", {}, {}),
    "p_f16-4.4.256-kv64": (4, 4, 256, 64, 40, T, "p_f16", {}, {}),
    # several splits, each window in LDS, COMBINE
    "lds-combine-8.8.32-kv512": (8, 8, 32, 512, 300, R, "lds", {}, {}),
    "lds-combine-8.8.32-kv512-T": (8, 8, 32, 512, 300, T, "lds", {}, {}),
    "lds-combine-16.4.64-kv600": (16, 4, 64, 600, 590, R, "lds", {}, {}),
    "lds-combine-16.4.64-kv600-T": (16, 4, 64, 600, 590, T, "lds", {}, {}),
    "lds-combine-32.8.128-kv1024": (32, 8, 128, 1024, 1000, R, "lds", {}, {}),
    "lds-combine-32.8.128-kv1024-T": (32, 8, 128, 1024, 1000, T, "lds", {}, {}),
    "lds-combine-32.8.64-per320": (32, 8, 64, 2560, 2500, R, "lds", {}, {}),
    # uneven splits in LDS (flash layout only: a transposed window in LDS is whole multiples of 8): the last split is shorter than `per`
    "lds-combine-short_last-32.8.128-kv1001": (32, 8, 128, 1001, 1000, R, "lds", {}, {}),
    "lds-combine-short_last-16.4.64-kv610": (16, 4, 64, 610, 600, R, "lds", {}, {}),
    "lds-combine-short_last-8.8.32-kv301": (8, 8, 32, 301, 300, R, "lds", {}, {}),
    "lds-combine-32.8.64-per320-T": (32, 8, 64, 2560, 2500, T, "lds", {}, {}),
    # global memory (plan_attn)
    "global-32.8.64-per321": (32, 8, 64, 2561, 2560, R, "global", {}, {}),
    "global-32.8.64-per321-T": (32, 8, 64, 2561, 2560, T, "global", {}, {}),
    "global-32.8.128-kv4096": (32, 8, 128, 4096, 4000, R, "global", {}, {}),
    "global-32.8.128-kv4096-T": (32, 8, 128, 4096, 4000, T, "global", {}, {}),
    "global-64.8.128-kv2048": (64, 8, 128, 2048, 2047, R, "global", {}, {}),
    "global-64.8.128-kv2048-T": (64, 8, 128, 2048, 2047, T, "global", {}, {}),
    "global-4.4.256-kv160": (4, 4, 256, 160, 100, R, "global", {}, {}),
    "global-p_f16-4.4.256-kv160-T": (4, 4, 256, 160, 100, T, "global", {}, {}),
    "global-unaligned-cache-32.8.128-kv256": (32, 8, 128, 256, 201, R, "global", {}, dict(k_off=8)),
    "global-unaligned-cache-32.8.128-kv1024-T": (32, 8, 128, 1024, 1000, T, "global", {}, dict(k_off=8)),
    "global-kv_lds0-32.8.128-kv256": (32, 8, 128, 256, 201, R, "global", dict(MI355Q_PLAN_KV_LDS=0), {}),
    "global-kv_lds0-p_f16-32.8.128-kv256-T": (32, 8, 128, 256, 201, T, "global", dict(MI355Q_PLAN_KV_LDS=0), {}),
    "global-kv_lds0-8.8.32-kv512-T": (8, 8, 32, 512, 300, T, "global", dict(MI355Q_PLAN_KV_LDS=0), {}),
    # run-time fallback: plan_attn_lds passes a transposed window with n_kv or per % 8 != 0 to plan_attn
    "fallback-p_f16-32.8.128-kv100-T": (32, 8, 128, 100, 90, T, "fallback", {}, {}),
    "fallback-combine-32.8.128-kv1000-per250-T": (32, 8, 128, 1000, 999, T, "fallback", {}, {}),
    "fallback-combine-8.8.32-kv300-per150-T": (8, 8, 32, 300, 299, T, "fallback", {}, {}),
}


def make_case(G, torch, name, **over):
    n_head, n_head_kv, hd, n_kv, slot, layout, form, envs, extra = FORM_CASES[name]
    kw = dict(extra); kw.update(over)
    kw["rope"] = dict(extra.get("rope", {}), **over.get("rope", {}))          # (the form's own rope mode, then the test's options)
    case = Case(G, torch, n_head, n_head_kv, hd, n_kv, kw.pop("slot", slot), layout, seed=kw.pop("seed", seed_of(name)), **kw)
    return case, form, envs


def run_form(G, torch, name, capfd=None, **over):
    """Build case `name` (with overrides), create its plan, assert the form (given capfd), run and check it.  Returns the error."""
    case, form, envs = make_case(G, torch, name, **over)
    try:
        if capfd is not None:
            capfd.readouterr()
            case.create(MI355Q_PLAN_VERBOSE=1, **envs)
            assert_form(capfd.readouterr().err, form, expected_splits(torch, case.n_head, case.n_kv), case)
        else:
            case.create(**envs)
        return run_and_check(case, form, name)
    finally:
        case.close()


@pytest.mark.parametrize("name", list(FORM_CASES))
def test_form(G, torch, capfd, name):
    if "short_last" in name:                                                      # (the id's claim: the window does not divide into its splits)
        n_head, n_kv = FORM_CASES[name][0], FORM_CASES[name][3]
        assert n_kv % expected_splits(torch, n_head, n_kv) != 0
    err = run_form(G, torch, name, capfd)
    print(f"{name}: error {err:.3e} of max|out|")


# ---- rope options on every f16 form -------------------------------------------------------------------------------------------------------
ROPE_FORMS = ["fa_seq-32.8.128-kv256", "p_f16-32.8.128-kv256", "lds-fa_exact0-32.8.128-kv256", "lds-combine-32.8.128-kv1024",
              "lds-combine-32.8.128-kv1024-T", "global-32.8.128-kv4096", "global-kv_lds0-p_f16-32.8.128-kv256-T", "fallback-p_f16-32.8.128-kv100-T",
              "fallback-combine-32.8.128-kv1000-per250-T"]


def rope_option(opt, hd, rng):
    """-> (rope dict overrides, freq_factors or None, rope position or None)"""
    if opt == "freq_factors":
        return {}, rng.uniform(1.0, 8.0, hd // 2).astype(np.float32), None
    if opt == "yarn":
        return dict(freq_scale=0.25, ext_factor=1.0, attn_factor=1.25, n_ctx_orig=4096), None, None
    if opt == "ndims_half_mode0":
        return dict(n_dims=hd // 2, mode=0), None, None
    if opt == "ndims_quarter_mode2":
        return dict(n_dims=hd // 4, mode=2), None, None
    if opt == "ndims_half_mode2_ff":
        return dict(n_dims=hd // 2, mode=2), rng.uniform(1.0, 8.0, hd // 4).astype(np.float32), None
    if opt == "pos100000":
        return {}, None, 100003
    raise AssertionError(opt)


ROPE_OPTS = ["freq_factors", "yarn", "ndims_half_mode0", "ndims_quarter_mode2", "ndims_half_mode2_ff", "pos100000"]


@pytest.mark.parametrize("opt", ROPE_OPTS)
@pytest.mark.parametrize("name", ROPE_FORMS)
def test_rope_options(G, torch, capfd, name, opt):
    rope, ff, pos = rope_option(opt, FORM_CASES[name][2], np.random.default_rng(seed_of(name, opt)))
    run_form(G, torch, name, capfd, rope=rope, ff=ff, pos=pos, seed=seed_of(name, opt))


# ---- masks on every form -----------------------------------------------------------------------------------------------------------------
MASK_FORMS = ["fa_seq-8.2.64-kv256-neox", "p_f16-8.2.64-kv256-neox", "lds-fa_exact0-32.8.128-kv256", "lds-combine-32.8.128-kv1024",
              "lds-combine-short_last-32.8.128-kv1001",
              "lds-combine-32.8.128-kv1024-T", "global-32.8.128-kv4096-T", "global-kv_lds0-32.8.128-kv256", "global-kv_lds0-8.8.32-kv512-T",
              "fallback-p_f16-32.8.128-kv100-T", "fallback-combine-32.8.128-kv1000-per250-T"]
MASK_PATTERNS = ["tail", "leading_run", "middle_run", "whole_split", "one_live_pos0"]


def mask_pattern(pattern, n_kv, slot, splits):
    """-> (live [n_kv], slot)"""
    live = np.zeros(n_kv, bool)
    if pattern == "one_live_pos0":
        live[0] = True
        return live, 0
    live[:slot + 1] = True
    if pattern == "leading_run":                                                 # a sliding window
        live[:slot // 3 + 1] = False
    elif pattern == "middle_run":                                                # another sequence's cells
        live[slot // 4:slot // 2] = False
    elif pattern == "whole_split":                                               # the second split, or half of a single one
        per = (n_kv + splits - 1) // splits
        lo, hi = (per, 2 * per) if slot >= 2 * per else (0, per) if splits > 1 else (slot // 4, 3 * slot // 4)
        assert hi <= slot
        live[lo:hi] = False
    return live, slot


@pytest.mark.parametrize("mask", ["f32", "f16"])
@pytest.mark.parametrize("pattern", MASK_PATTERNS)
@pytest.mark.parametrize("name", MASK_FORMS)
def test_masks(G, torch, capfd, name, pattern, mask):
    n_head, _, _, n_kv, slot, _, _, _, _ = FORM_CASES[name]
    live, slot = mask_pattern(pattern, n_kv, slot, expected_splits(torch, n_head, n_kv))
    run_form(G, torch, name, capfd, mask=mask, live=live, slot=slot, seed=seed_of(name, pattern, mask))


@pytest.mark.parametrize("name", MASK_FORMS)
def test_no_mask(G, torch, capfd, name):
    """No mask: every position of the window is live (the rows beyond it hold garbage)."""
    n_kv = FORM_CASES[name][3]
    run_form(G, torch, name, capfd, mask=None, slot=n_kv - 1, seed=seed_of(name, "nomask"))


# ---- the LDS / global boundary, found through plan_create ----------------------------------------------------------------------------------
def lds_accepts(G, torch, capfd, case, n_kv):
    case.attn["n_kv"] = n_kv
    capfd.readouterr()
    with env(MI355Q_PLAN_VERBOSE=1, **FORM_ENV):
        G.Plan(case.stages).close()
    (line,) = parse_forms(capfd.readouterr().err)
    return line[3]


@pytest.mark.parametrize("shape", [(32, 8, 128), (64, 8, 128)], ids=["32.8.128", "64.8.128"])
def test_lds_boundary(G, torch, capfd, shape):
    """The largest window whose splits still land in the LDS (bisected over plan_create alone), then the last window in and the first out."""
    n_head, n_head_kv, hd = shape
    top = 16384
    probe = Case(G, torch, n_head, n_head_kv, hd, top, 0, R, seed=1)
    lo, hi = 256, top
    assert lds_accepts(G, torch, capfd, probe, lo) and not lds_accepts(G, torch, capfd, probe, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lds_accepts(G, torch, capfd, probe, mid) else (lo, mid)
    splits = expected_splits(torch, n_head, lo)
    print(f"{shape}: largest LDS window {lo} ({splits} splits of {(lo + splits - 1) // splits})")
    assert splits > 1
    for n_kv, form in ((lo, "lds"), (hi, "global")):
        case = Case(G, torch, n_head, n_head_kv, hd, n_kv, n_kv - 1, R, seed=seed_of(shape, n_kv))
        try:
            capfd.readouterr()
            case.create(MI355Q_PLAN_VERBOSE=1)
            assert_form(capfd.readouterr().err, form, expected_splits(torch, n_head, n_kv), case)
            run_and_check(case, form, f"{shape} n_kv {n_kv}")
        finally:
            case.close()


# ---- n_kv_dev: the per-run window ---------------------------------------------------------------------------------------------------------
def n_kv_dev_bench_case(G, torch, pos, n_kv_dev):
    """bench.py's shape and convention: one plan sized for n_kv 1024 with a transposed V, window n_kv_dev, causal mask row, rows past the window NaN."""
    return Case(G, torch, 32, 8, 128, 1024, pos, T, mask="f32", n_kv_dev=n_kv_dev, seed=seed_of("bench", pos, n_kv_dev))


def nkv_dev_form(w, splits=4):
    """The form a transposed-V window of w positions over `splits` LDS splits runs in: plan_attn_lds, or plan_attn when per or w is not a multiple
    of 8 (the run-time fallback)."""
    per = (w + splits - 1) // splits
    return "fallback" if (per | w) & 7 else "lds"


NKV_DEV = {}
for p_, w_ in [(0, 32), (31, 32), (32, 64), (255, 256), (256, 288), (700, 704), (1023, 1024), (0, 1), (4, 5), (8, 9), (1000, 5000)]:
    tag = {1: "-empty_splits", 5: "-last_split_empty", 9: "-last_split_empty", 5000: "-clamped"}.get(w_, "")
    NKV_DEV[f"{nkv_dev_form(min(w_, 1024))}-pos{p_}-win{w_}{tag}"] = (p_, w_)


@pytest.mark.parametrize("name", list(NKV_DEV))
def test_n_kv_dev_bench_shape(G, torch, capfd, name):
    """bench.py's plan: transposed V, n_kv 1024 = 4 LDS splits, run over shorter windows (padded to 32 as bench.py does), which change `per` at run
    time; n_kv_dev > n_kv is clamped to n_kv.  Windows of 1, 5 and 9 positions leave splits with no position (cnt == 0) before COMBINE, but with
    per = 1, 2, 3 (not multiples of 8) plan_attn_lds hands them to plan_attn at run time: the ids say "fallback" and the empty splits are
    plan_attn's.  plan_attn_lds meets empty and short splits in test_n_kv_dev_flash_layout_splits."""
    pos, w = NKV_DEV[name]
    case = n_kv_dev_bench_case(G, torch, pos, w)
    try:
        form = name.split("-")[0]
        assert case.w == min(1024, w) and form == nkv_dev_form(case.w)
        capfd.readouterr()
        case.create(MI355Q_PLAN_VERBOSE=1)
        text = capfd.readouterr().err
        assert parse_forms(text) == [(1024, 4, 256, True, False)]
        assert_form(text, form, 4, case)
        run_and_check(case, form, name)
    finally:
        case.close()


NKV_DEV_ROWS = {"win1-empty_splits": 1, "win5-last_split_empty": 5, "win9-last_split_empty": 9, "win300": 300, "win301-short_last_split": 301,
                "win1023-short_last_split": 1023}


@pytest.mark.parametrize("name", list(NKV_DEV_ROWS))
def test_n_kv_dev_flash_layout_splits(G, torch, capfd, name):
    """A flash-layout (rows_v) plan sized for n_kv 1024 = 4 LDS splits of 256, run over shorter windows: plan_attn_lds itself runs splits with no
    position (cnt == 0: n_kv_dev 1, and 5 / 9 whose last split starts at or past the window) and last splits shorter than `per` (301, 1023), then
    COMBINE merges them.  (No run-time fallback exists for this layout.)"""
    w = NKV_DEV_ROWS[name]
    case = Case(G, torch, 32, 8, 128, 1024, w - 1, R, mask="f32", n_kv_dev=w, seed=seed_of("rows_dev", w))
    try:
        per = (w + 3) // 4
        assert (3 * per >= w) == ("empty" in name) and (w % per != 0 and 3 * per < w) == ("short_last" in name)
        capfd.readouterr()
        case.create(MI355Q_PLAN_VERBOSE=1)
        assert parse_forms(capfd.readouterr().err) == [(1024, 4, 256, True, False)]
        run_and_check(case, "lds", name)
    finally:
        case.close()


@pytest.mark.parametrize("mask", ["f16", None], ids=["mask_f16", "no_mask"])
@pytest.mark.parametrize("w", [1, 32, 100, 201, 256])
def test_n_kv_dev_flash_sequential(G, torch, capfd, w, mask):
    """A flash-layout plan sized for n_kv 256 (fa_seq) run over shorter windows: glue.flash_attn_ext's bits over the shortened window."""
    case = Case(G, torch, 32, 8, 128, 256, w - 1, R, mask=mask, n_kv_dev=w, seed=seed_of("fa_dev", w, mask))
    try:
        capfd.readouterr()
        case.create(MI355Q_PLAN_VERBOSE=1)
        assert parse_forms(capfd.readouterr().err) == [(256, 1, 256, True, True)]
        run_and_check(case, "fa_seq", f"window {w}")
    finally:
        case.close()


# ---- rope options on the q8_0 / q4_0 stage -----------------------------------------------------------------------------------------------
def quant_rope_case(G, torch, kv, opt, n_kv=256, slot=200):
    """test_gpu_plan_quant_kv.Stage with the rope option `opt`: returns the stage, its rope position set on the device."""
    from test_gpu_plan_quant_kv import Stage
    rng = np.random.default_rng(seed_of(kv, opt))
    rope, ff, pos = rope_option(opt, 128, rng)

    class RStage(Stage):
        def rope(self, t, n):
            r = self.rp
            return self.G.op_rope(t.view(1, 1, n, self.hd), self.posd, r["n_dims"], r["mode"], freq_factors=self.ffd, n_ctx_orig=r["n_ctx_orig"],
                                  freq_base=500000.0, freq_scale=r["freq_scale"], ext_factor=r["ext_factor"], attn_factor=r["attn_factor"])

    st = RStage(G, torch, kv, 32, 8, 128, n_kv, slot, "f16", mode=rope.get("mode", 0), seed=seed_of(kv, opt))
    st.rp = dict(n_dims=128, mode=0, n_ctx_orig=8192, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0)
    st.rp.update(rope)
    st.ffd = None if ff is None else torch.from_numpy(ff).cuda()
    st.attn["rope"] = dict(st.rp, freq_base=500000.0)
    st.attn["freq_factors"] = st.ffd
    if pos is not None:
        st.posd.fill_(pos)
    return st


@pytest.mark.parametrize("opt", ROPE_OPTS)
@pytest.mark.parametrize("kv", ["q8_0", "q4_0"])
def test_quantized_stage_rope_options(G, torch, kv, opt):
    """One split: the stored blocks are op_cpy(op_rope(k)) byte for byte and the output is glue.flash_attn_ext_q8_0's bits."""
    st = quant_rope_case(G, torch, kv, opt)
    with env(**FORM_ENV):                                                        # (one split: the CPU's bits)
        st.run()
    kc, vc = st.check_stores()
    got, ref = st.got(), st.reference(kc, vc)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.abs(got - ref).max()


# ---- clean refusals (plan_create only, nothing launched) ----------------------------------------------------------------------------------
REFUSALS = {
    "head_dim80": dict(hd=80, n_head=4, n_head_kv=4, match="bad head geometry"),
    "head_dim16": dict(hd=16, n_head=4, n_head_kv=4, match="bad head geometry"),
    "head_dim288": dict(hd=288, n_head=4, n_head_kv=4, match="bad head geometry"),
    "n_head_not_multiple_of_n_head_kv": dict(hd=64, n_head=6, n_head_kv=4, match="bad head geometry"),
    "more_heads_than_cus": dict(hd=32, n_head=None, n_head_kv=1, match="more heads than CUs"),
    "rope_mode1": dict(hd=64, n_head=4, n_head_kv=4, rope=dict(mode=1), match="rope mode"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(G, torch, name):
    r = dict(REFUSALS[name])
    hd = r["hd"]; n_head = r["n_head"] or n_cu(torch) + 4; n_head_kv = r["n_head_kv"]
    n_kv = 64
    # (a geometry the Case builder cannot lay out itself: build a valid one of the same sizes, then set the refused fields)
    case = Case(G, torch, n_head_kv, n_head_kv, 32, n_kv, 10, R, seed=7)
    q = torch.zeros((1, n_head * hd), dtype=torch.float32, device="cuda"); kv_ = torch.zeros((1, n_head_kv * hd), dtype=torch.float32, device="cuda")
    case.attn.update(head_dim=hd, n_head=n_head, n_head_kv=n_head_kv, q=q, k=kv_, v=kv_.clone(), out=torch.zeros_like(q), k_nb_head=hd * 2,
                     rope=dict(case.attn["rope"], n_dims=min(hd, 64), **r.get("rope", {})))
    with pytest.raises(G.Mi355qError, match=r["match"]):
        G.Plan(case.stages)
