"""Host logic of the Q4_1 / Q5_0 / Q5_1 / IQ4_NL KV cache that needs no GPU: the stage flags of include/mi355q.h, the Python mirror's names for
them, the block sizes, and the API version (unchanged: no function or structure changed)."""
import re

import pytest

import kvq_ref
from conftest import ROOT

HEADER = (ROOT / "include" / "mi355q.h").read_text()


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9A-Fa-f]+|\d+)\b", HEADER, re.M)
    assert m, f"{name} is not defined in include/mi355q.h"
    return int(m.group(1), 0)


@pytest.mark.parametrize("kv", list(kvq_ref.TYPES))
def test_header_defines_the_stage_flag_and_the_mirror_maps_the_name(kv):
    import ggml_mi355 as g
    type_id, bb, flag = kvq_ref.TYPES[kv]
    assert _define(f"MI355Q_STAGE_KV_{kv.upper()}") == flag
    assert g._STAGE_KV[kv] == flag
    assert g.KV_BLOCK[kv] == (bb, type_id)
    assert _define(f"MI355Q_TYPE_{kv.upper()}") == type_id


def test_flags_are_distinct_bits_after_the_existing_ones():
    import ggml_mi355 as g
    assert _define("MI355Q_STAGE_KV_Q8_0") == 0x4 and _define("MI355Q_STAGE_KV_Q4_0") == 0x8
    flags = [v for k, v in g._STAGE_KV.items() if k != "f16"]
    assert len(flags) == 6 and all(f & (f - 1) == 0 for f in flags) and len(set(flags)) == 6
    assert sorted(flags) == [0x4, 0x8, 0x10, 0x20, 0x40, 0x80]
    assert g._STAGE_KV["f16"] == 0
    assert _define("MI355Q_API_VERSION") == 3


def test_header_states_the_block_sizes_and_the_older_library_caveat():
    block = HEADER[HEADER.index("ATTN stages over a QUANTIZED KV cache"):HEADER.index("#define MI355Q_STAGE_KV_Q8_0")]
    for kv, (_, bb, _) in kvq_ref.TYPES.items():
        assert re.search(rf"{bb} \({kv}\)", block), kv
    assert "older" in block and "mi355q_op_flash_attn_ext" in block
