"""The Python mirror of the decode plan's mixed K / V attention stage flags (no GPU): `kv=` / `kv_v=` of an attention stage dict become the
MI355Q_STAGE_KV_* / MI355Q_STAGE_KVV_* values include/mi355q.h declares; unknown names are refused; the V bits collide with no other stage flag."""
import re

import pytest

from conftest import ROOT

NAMES = ["f16", "q8_0", "q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl"]


@pytest.fixture(scope="module")
def header():
    """{name: value} of every `#define MI355Q_STAGE_* <number>` of include/mi355q.h."""
    text = (ROOT / "include" / "mi355q.h").read_text()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(MI355Q_STAGE_\w+)\s+(0x[0-9a-fA-F]+|\d+)\b", text, re.M)}


def attn_stage(**kw):
    import torch
    z = torch.zeros(8)
    a = dict(q=z, k=z, v=z, pos=z, k_cache=z, v_cache=z, k_dst=z, v_dst=z, out=z, k_nb_pos=0, k_nb_head=0, v_nb_pos=0, v_nb_dim=0, v_nb_head=0,
             v_dst_nb=0, n_head=1, n_head_kv=1, head_dim=32, n_kv=1, scale=1.0)
    a.update(kw)
    return dict(attn=a, no_plain=True)


def flags_of(**kw):
    import ggml_mi355 as g
    arr, _keep = g._stage_array([attn_stage(**kw)])
    return arr[0].flags & ~g.STAGE_NO_PLAIN


def test_header_declares_a_v_bit_per_type_above_the_k_bits(header):
    vbits = [header[f"MI355Q_STAGE_KVV_{n.upper()}"] for n in NAMES]
    assert all(v & (v - 1) == 0 and v > header["MI355Q_STAGE_KV_IQ4_NL"] for v in vbits) and len(set(vbits)) == 7
    # ... and they collide with no other stage flag (GEMV / ATTN are stage kinds, not flags)
    others = [v for k, v in header.items() if not k.startswith("MI355Q_STAGE_KVV_") and k not in ("MI355Q_STAGE_GEMV", "MI355Q_STAGE_ATTN")]
    assert len(others) >= 8
    for v in vbits:
        assert all(v & o == 0 for o in others), hex(v)


@pytest.mark.parametrize("kv_v", [None] + NAMES)
@pytest.mark.parametrize("kv", NAMES)
def test_names_map_to_the_header_values(header, kv, kv_v):
    want = 0 if kv == "f16" else header[f"MI355Q_STAGE_KV_{kv.upper()}"]
    if kv_v is not None:
        want |= header[f"MI355Q_STAGE_KVV_{kv_v.upper()}"]
    assert flags_of(kv=kv, kv_v=kv_v) == want
    if kv_v is None:
        assert flags_of(kv=kv) == want                                       # (no kv_v key at all: as before)


def test_default_is_f16_without_a_v_bit():
    assert flags_of() == 0


@pytest.mark.parametrize("kw", [dict(kv="q8_1"), dict(kv="q8_0", kv_v="q6_K"), dict(kv="f16", kv_v="f32"), dict(kv="q4_0", kv_v=""),
                                dict(kv="bf16"), dict(kv="q8_0", kv_v="bf16")], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_unknown_names_are_refused(kw):
    with pytest.raises(ValueError, match="bf16" if "bf16" in kw.values() else "must be one of"):
        flags_of(**kw)
