"""ggml_mi355._stage_array: the mi355q_stage records ggml_mi355.Plan hands to mi355q_plan_create, built here from CPU tensors (the helper reads
addresses, shapes and dtypes only; no library call, no device).  What is pinned: the value ids (x_id, x1_id, y_ids, sum_id; q_id, k_id, v_id,
out_id of an attention stage) land in the struct fields of include/mi355q.h, x_out and sum_out carry the tensors' addresses, and a stage
that names none of them is byte-identical to what the wrapper built before it knew the ids (all of them 0)."""
import ctypes as C

import pytest
import torch

import oracle


@pytest.fixture(scope="module")
def G():
    import ggml_mi355 as g
    if not g.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return g


def vec(n, dtype=torch.float32):
    return torch.zeros((1, n), dtype=dtype)


def weight(G, t, m, k):
    return G.QWeight(t, torch.zeros(m * G.row_size(t, k) + 64, dtype=torch.uint8), m, k)


def raw(st):
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


def test_gemv_ids_and_outputs_land_in_the_struct(G):
    K = 512
    w = [weight(G, oracle.Q4_K, m, K) for m in (64, 32, 96)]
    x, x1, nw, so, xo = (vec(K) for _ in range(5))
    ys = [vec(m) for m in (64, 32, 96)]
    arr, keep = G._stage_array([dict(ws=w, ys=ys, x=x, x1=x1, x_kind=G.X_NORM, norm_w=nw, eps=1e-5, sum_out=so, x_out=xo, no_plain=True,
                                     x_id=7, x1_id=-3, y_ids=[11, 0, 2 ** 40 + 5], sum_id=9)])
    st = arr[0]
    assert (st.kind, st.n_mats, st.k, st.x_kind, st.flags) == (G.STAGE_GEMV, 3, K, G.X_NORM, G.STAGE_NO_PLAIN)
    assert (st.x_id, st.x1_id, st.sum_id) == (7, -3, 9)
    assert list(st.y_id) == [11, 0, 2 ** 40 + 5, 0]
    assert (st.x, st.x1, st.norm_w, st.sum_out, st.x_out) == (x.data_ptr(), x1.data_ptr(), nw.data_ptr(), so.data_ptr(), xo.data_ptr())
    for j, (wj, y) in enumerate(zip(w, ys)):
        m = st.mats[j]
        assert (m.type, m.w, m.w_stride, m.y, m.m) == (oracle.Q4_K, wj.data.data_ptr(), wj.row_bytes, y.data_ptr(), wj.M)
    assert keep and len(arr) == 1


def test_sub_vector_operand_carries_its_own_address(G):
    """A view into a fused output: the address is the view's, K its length."""
    fused = vec(3072)
    w = weight(G, oracle.Q8_0, 40, 512)
    arr, _ = G._stage_array([dict(ws=[w], ys=[vec(40)], x=fused[:, 2048:2560], x_id=5)])
    assert arr[0].x == fused.data_ptr() + 2048 * 4 and arr[0].k == 512 and arr[0].x_id == 5


def test_defaults_are_all_zero_and_byte_identical(G):
    K = 256
    w = weight(G, oracle.Q4_K, 32, K)
    x, y = vec(K), vec(32)
    plain, _ = G._stage_array([dict(ws=[w], ys=[y], x=x)])
    named, _ = G._stage_array([dict(ws=[w], ys=[y], x=x, x_id=0, x1_id=0, y_ids=None, sum_id=0)])
    tup, _ = G._stage_array([([w], x, [y], False)])
    st = plain[0]
    assert (st.x_id, st.x1_id, st.sum_id, list(st.y_id)) == (0, 0, 0, [0, 0, 0, 0])
    assert not st.x_out and not st.sum_out and not st.x1
    assert raw(plain[0]) == raw(named[0])
    assert (tup[0].x_id, tup[0].x1_id, tup[0].sum_id, list(tup[0].y_id), tup[0].x, tup[0].k) == (0, 0, 0, [0, 0, 0, 0], x.data_ptr(), K)   # the tuple form
    with pytest.raises(AssertionError):
        G._stage_array([dict(ws=[w], ys=[y], x=x, y_ids=[1, 2])])      # one id per matrix


def test_attention_ids_land_in_the_struct(G):
    hd, nh = 64, 4
    q, k, v, out = (vec(nh * hd) for _ in range(4))
    cache = torch.zeros((64, nh * hd), dtype=torch.float16)
    dst = torch.zeros(2, dtype=torch.int64)
    base = dict(q=q, k=k, v=v, pos=torch.zeros(1, dtype=torch.int32), k_cache=cache, v_cache=cache, k_nb_pos=nh * hd * 2, k_nb_head=hd * 2,
                v_nb_pos=nh * hd * 2, v_nb_dim=2, v_nb_head=hd * 2, k_dst=dst[0:1], v_dst=dst[1:2], v_dst_nb=2,
                mask=torch.zeros(64, dtype=torch.float16), n_head=nh, n_head_kv=nh, head_dim=hd, n_kv=37, scale=0.125, out=out)
    arr, keep = G._stage_array([dict(attn=dict(base, q_id=5, k_id=6, v_id=-7, out_id=8))])
    at = arr[0].attn.contents
    assert arr[0].kind == G.STAGE_ATTN
    assert (at.q_id, at.k_id, at.v_id, at.out_id) == (5, 6, -7, 8)
    assert (at.q, at.k, at.v, at.out, at.mask_f16, at.n_kv) == (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, 37)
    arr0, keep0 = G._stage_array([dict(attn=base)])
    at0 = arr0[0].attn.contents
    assert (at0.q_id, at0.k_id, at0.v_id, at0.out_id) == (0, 0, 0, 0)
    at.q_id = at.k_id = at.v_id = at.out_id = 0
    assert raw(at) == raw(at0)
