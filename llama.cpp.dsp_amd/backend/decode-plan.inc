// decode-plan.inc -- included by ggml-mi355.cpp: turns the N = 1 decode graph of a llama-architecture model into ONE persistent launch
// (mi355q_plan_*, csrc/plan.hip) -- the MI355X-first counterpart of the reference's whole-step CUDA-graph replay (ggml-cuda.cu:2646-2781).
//
// The graph the reference builds per generated token (src/llama-model.cpp llm_build_llama; src/llama-graph.cpp build_norm, build_attn,
// build_attn_mha, build_ffn) is a chain of quantized MUL_MATs with small glue ops between them.  The matcher below recognises, by DATAFLOW
// (not by node position), the sub-expressions a plan stage computes:
//
//   GEMV   a group of <= 4 quantized MUL_MATs on the same activation tensor X, where X is
//            MUL(RMS_NORM(T), w)   with T = ADD(a, b) or any vector    -> MI355Q_X_NORM       (ADD, RMS_NORM, MUL folded into the stage's prologue)
//            MUL(UNARY(a), b)      with SILU / RELU / SIGMOID          -> MI355Q_X_UNARY_MUL  (UNARY, MUL folded)
//            anything else                                              -> MI355Q_X_PLAIN
//   ATTN   CONT(PERMUTE(MUL_MAT(v, SOFT_MAX(MUL_MAT(k, PERMUTE(ROPE(q))), mask)))) or FLASH_ATTN_EXT(PERMUTE(ROPE(q)), k, v, mask) together with the
//          ROPE of k and the two CPY nodes that store this token's K / V rows in the caches k and v view.
//
// Every compute node of the graph must fall into a stage, except a prefix and a suffix of the node list, which are issued node by node before / after
// the launch (e.g. the layer-output ADD a scheduler split ends with); tensors they exchange with the plan are stored as plain f32.  Anything
// else -- more than one token, an op outside the patterns, a weight type without a streaming kernel -- makes the matcher decline, and
// graph_compute falls back to issuing nodes (with launch graphs and fusions) as before.
//
// Memory: inside the launch, intermediates live in the plan's private granule buffers, never in the graph allocator's memory, so the allocator's
// reuse of dead tensors cannot alias anything; operands are identified by their addresses at build time only.

struct mi355_plan_build {
    std::vector<mi355q_stage> stages;
    std::vector<mi355q_attn *> attns;                // owned
    std::vector<int> anchor;                         // node index that orders the stage
    std::vector<std::vector<const struct ggml_tensor *>> outs;   // per stage: tensors it produces (for the plain-store decision)
    std::vector<std::vector<int>> nodes;             // per stage: the graph nodes it covers
    ~mi355_plan_build() { for (auto * a : attns) delete a; }
};

static const struct ggml_tensor * mi355_skip_views(const struct ggml_tensor * t) {
    while (t && mi355_is_view_op(t) && t->op != GGML_OP_NONE && t->src[0]) t = t->src[0];
    return t;
}
static bool mi355_is_vec_f32(const struct ggml_tensor * t) {      // n contiguous floats
    return t && t->type == GGML_TYPE_F32 && ggml_is_contiguous(t) && t->data && ((uintptr_t) t->data & 15) == 0;
}
static bool mi355_plan_mat(const struct ggml_tensor * n) {          // a quantized MUL_MAT with one activation row, streamable by the plan
    if (n->op != GGML_OP_MUL_MAT || !mi355_is_quant(n->src[0]->type)) return false;
    const struct ggml_tensor * w = n->src[0], * x = n->src[1];
    if (ggml_nelements(x) != x->ne[0] || !mi355_is_vec_f32(x) || !mi355_is_vec_f32(n) || ggml_nelements(n) != n->ne[0]) return false;
    if (w->ne[2] != 1 || w->ne[3] != 1 || mi355_root(w)->ne[0] != w->ne[0] || w->nb[0] != ggml_type_size(w->type)) return false;
    if (mi355q_weights_are_planar((int) w->type, w->ne[0]) != 1 || mi355_q80_canonical(w) || (w->nb[1] % 16) || ((uintptr_t) w->data % 16)) return false;
    switch (w->type) {                                       // (which mixes of these have a kernel instantiation is mi355q_plan_create's call: a refusal declines the plan)
    case GGML_TYPE_Q4_K: case GGML_TYPE_Q5_K: case GGML_TYPE_Q6_K: case GGML_TYPE_Q8_0: case GGML_TYPE_Q4_0: case GGML_TYPE_IQ4_NL: case GGML_TYPE_IQ4_XS:
    case GGML_TYPE_IQ3_S: case GGML_TYPE_IQ3_XXS: return true;
    default: return false;
    }
}

struct mi355_plan_matcher {
    struct ggml_cgraph * g;
    std::unordered_map<const struct ggml_tensor *, int> producer;
    std::vector<char> covered;
    std::vector<int> cpy_ordinal;                    // node index -> ordinal among the non-empty CPY nodes (dest_table slot), -1 otherwise
    std::vector<char> is_mat;                        // node index -> mi355_plan_mat(node), evaluated once
    std::vector<int> mats, cpys;                     // ascending node indices of the plan matmuls / the non-empty CPY nodes (the searches below walk these, not the graph)
    std::unordered_map<const struct ggml_tensor *, int> n_uses;   // consumers inside this graph (through views)
    std::unordered_set<const struct ggml_tensor *> mask_casts;   // F16 copies of the f32 mask whose attention stages read the source instead
    void ** dest_table;
    explicit mi355_plan_matcher(struct ggml_cgraph * cgraph, void ** dest) : g(cgraph), covered((size_t) cgraph->n_nodes, 0), cpy_ordinal((size_t) cgraph->n_nodes, -1), dest_table(dest) {
        int n_cpy = 0;
        producer.reserve((size_t) g->n_nodes * 2); n_uses.reserve((size_t) g->n_nodes * 4); is_mat.assign((size_t) g->n_nodes, 0);
        for (int i = 0; i < g->n_nodes; ++i) {
            producer[g->nodes[i]] = i;
            if (mi355_plan_mat(g->nodes[i])) { is_mat[(size_t) i] = 1; mats.push_back(i); }
            if (g->nodes[i]->op == GGML_OP_CPY && !ggml_is_empty(g->nodes[i])) { cpy_ordinal[(size_t) i] = n_cpy++; cpys.push_back(i); }
            for (int s = 0; s < GGML_MAX_SRC; ++s) for (const struct ggml_tensor * t = g->nodes[i]->src[s]; t; t = t->view_src) ++n_uses[t];
        }
    }
    bool single_use(const struct ggml_tensor * t) const { auto it = n_uses.find(t); return !(t->flags & GGML_TENSOR_FLAG_OUTPUT) && it != n_uses.end() && it->second == 1; }
    // GET_ROWS(a, ids) of a ONE-row f32 tensor with ONE index can only return that row: llm_build_llama inserts exactly this in the last layer
    // (cur = get_rows(cur, inp_out_ids), inpSA = get_rows(inpSA, inp_out_ids), src/llama-model.cpp:4512-4514) also when a single token is decoded.
    // Such a node is an alias of its source inside a stage; the consumer's operand is then the source's value.
    bool is_identity_rows(const struct ggml_tensor * t) const {
        if (!t || t->op != GGML_OP_GET_ROWS || idx(t) < 0 || covered[(size_t) idx(t)]) return false;
        const struct ggml_tensor * a = t->src[0], * ids = t->src[1];
        return a && ids && a->type == GGML_TYPE_F32 && t->type == GGML_TYPE_F32 && ggml_is_contiguous(a) && ggml_nelements(a) == a->ne[0] && ggml_nelements(t) == a->ne[0] &&
               ids->type == GGML_TYPE_I32 && ggml_nelements(ids) == 1 && single_use(t);
    }
    const struct ggml_tensor * through_rows(const struct ggml_tensor * t) const { return is_identity_rows(t) ? t->src[0] : t; }
    // how many plan matmuls of the graph read X as their activations (all of them are folded into stages on X's prologue)
    int mat_readers(const struct ggml_tensor * X) const { int c = 0; for (int i : mats) if (g->nodes[i]->src[1] == X) ++c; return c; }
    // X = the vector a stage's prologue forms.  It exists only as the stage's quantized LDS image unless somebody besides the stage's matrices
    // reads it -- another node of the graph, or the caller after the graph (an OUTPUT flag; llama.cpp reads result_norm back as the embeddings
    // without flagging it, so the vector behind the graph's last matmul is always kept): then the stage also stores it (mi355q_stage.x_out).
    bool needs_x_out(const struct ggml_tensor * X, const struct ggml_tensor * last_mat) const {
        auto it = n_uses.find(X);
        const int uses = it == n_uses.end() ? 0 : it->second;
        if ((X->flags & GGML_TENSOR_FLAG_OUTPUT) || uses != mat_readers(X)) return true;
        return last_mat == g->nodes[g->n_nodes - 1] || (last_mat->flags & GGML_TENSOR_FLAG_OUTPUT);
    }
    int idx(const struct ggml_tensor * t) const { auto it = producer.find(t); return it == producer.end() ? -1 : it->second; }
    // value id of a tensor: the index (+1) of the compute node that produces its data, 0 for leafs / graph inputs (plain operands).  The graph
    // allocator hands one address to several intermediates (K's projection reuses the dead pre-rope Q's block, V's reuses K's), so addresses
    // cannot identify the operands of a plan that consumes k after v has been produced (include/mi355q.h, VALUE IDS).
    int64_t vid(const struct ggml_tensor * t) const { t = mi355_skip_views(t); const int i = t ? idx(t) : -1; return i >= 0 ? i + 1 : 0; }
    std::vector<int> * cur = nullptr;               // node list of the stage being matched
    void cover(const struct ggml_tensor * t) { const int i = idx(t); if (i >= 0) { covered[(size_t) i] = 1; if (cur) cur->push_back(i); } }

    // the quantized MUL_MAT node whose output (through views) is t, or nullptr
    const struct ggml_tensor * mat_behind(const struct ggml_tensor * t) const {
        t = mi355_skip_views(t);
        const int i = t ? idx(t) : -1;
        return i >= 0 && is_mat[(size_t) i] ? t : nullptr;
    }

    // ---- attention of one token; `top` is the node whose data the output projection reads (the CONT, or the FLASH_ATTN_EXT node)
    bool match_attn(const struct ggml_tensor * top, mi355_plan_build & b) {
        const struct ggml_tensor * fa = nullptr, * kq = nullptr, * sm = nullptr, * kqv = nullptr, * kview, * vview, * qperm, * mask;
        float scale, max_bias, softcap = 0.0f;
        if (top->op == GGML_OP_FLASH_ATTN_EXT) {
            fa = top; qperm = fa->src[0]; kview = fa->src[1]; vview = fa->src[2]; mask = fa->src[3];
            memcpy(&scale, (const float *) fa->op_params + 0, 4); memcpy(&max_bias, (const float *) fa->op_params + 1, 4); memcpy(&softcap, (const float *) fa->op_params + 2, 4);
        } else {
            if (top->op != GGML_OP_CONT) return false;
            kqv = mi355_skip_views(top->src[0]);
            if (!kqv || kqv->op != GGML_OP_MUL_MAT || kqv->src[0]->type != GGML_TYPE_F16) return false;
            vview = kqv->src[0]; sm = kqv->src[1];
            if (sm->op != GGML_OP_SOFT_MAX) return false;
            kq = sm->src[0]; mask = sm->src[1];
            if (kq->op != GGML_OP_MUL_MAT || kq->src[0]->type != GGML_TYPE_F16) return false;
            kview = kq->src[0]; qperm = kq->src[1];
            memcpy(&scale, (const float *) sm->op_params + 0, 4); memcpy(&max_bias, (const float *) sm->op_params + 1, 4);
        }
        if (max_bias != 0.0f || softcap != 0.0f) return false;
        // the cache: f16, or (flash graphs only) both K and V in blocks of one of Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 / IQ4_NL (-ctk T -ctv T): the stage flag MI355Q_STAGE_KV_*
        // Mixed types (-ctk A -ctv B, each of f16 or a block type; flash graphs only): K's type keeps the MI355Q_STAGE_KV_* bit and a MI355Q_STAGE_KVV_* bit names
        // V's -- only with MI355_PLAN_KV_MIXED=1 in the environment (off by default: DESIGN.md 5.6); otherwise such a graph runs node by node.
        const enum ggml_type kvt = kview->type, vvt = vview->type;
        const bool kv_quant = fa && mi355_kv_block_type(kvt), v_quant = fa && mi355_kv_block_type(vvt);
        const bool kv_mixed = vvt != kvt;
        if (kv_mixed) { const char * e = getenv("MI355_PLAN_KV_MIXED"); if (!fa || !e || atoi(e) != 1) return false; }
        const size_t kv_nb0 = kv_quant ? ggml_type_size(kvt) : 2, v_nb0 = v_quant ? ggml_type_size(vvt) : 2;     // bytes per element (f16) or per 32-block, per side
        if ((kvt != GGML_TYPE_F16 && !kv_quant) || (vvt != GGML_TYPE_F16 && !v_quant) || !kview->view_src || !vview->view_src || kview->nb[0] != kv_nb0) return false;
        const struct ggml_tensor * rq = mi355_skip_views(qperm);
        if (!rq || rq->op != GGML_OP_ROPE) return false;
        const struct ggml_tensor * qm = mat_behind(rq->src[0]);
        if (!qm) return false;
        const int64_t hd = kview->ne[0], n_kv = kview->ne[1], n_head_kv = kview->ne[2];
        if (rq->ne[0] != hd || rq->ne[2] != 1 || rq->ne[3] != 1) return false;                  // one token
        const int64_t n_head = rq->ne[1];
        if (ggml_nelements(qm) != n_head * hd || n_head_kv < 1 || n_head % n_head_kv) return false;
        // the cache stores of this token: the CPY nodes whose destination views the same cache tensors
        const struct ggml_tensor * ck = nullptr, * cv = nullptr;
        for (int i : cpys) {
            const struct ggml_tensor * n = g->nodes[i];
            if (!n->src[1]->view_src) continue;
            if (n->src[1]->view_src == kview->view_src) { if (ck) return false; ck = n; }
            else if (n->src[1]->view_src == vview->view_src) { if (cv) return false; cv = n; }
        }
        if (!ck || !cv || ck->src[1]->type != kvt || cv->src[1]->type != vvt) return false;                            // each store's destination has its own side's type
        if ((kv_quant && ck->src[0]->type != GGML_TYPE_F32) || (v_quant && cv->src[0]->type != GGML_TYPE_F32)) return false;       // CPY f32 -> the cache type
        const struct ggml_tensor * rk = mi355_skip_views(ck->src[0]);
        if (!rk || rk->op != GGML_OP_ROPE || rk->src[1] != rq->src[1] || rk->src[2] != rq->src[2]) return false;
        if (memcmp(rk->op_params, rq->op_params, sizeof(rk->op_params)) != 0) return false;
        const struct ggml_tensor * km = mat_behind(rk->src[0]), * vm = mat_behind(cv->src[0]);
        if (!km || !vm || ggml_nelements(km) != n_head_kv * hd || ggml_nelements(vm) != n_head_kv * hd) return false;
        if (ggml_nelements(ck->src[1]) != n_head_kv * hd || ggml_nelements(cv->src[1]) != n_head_kv * hd) return false;
        const int32_t * rp = (const int32_t *) rq->op_params;
        if ((rp[2] != 0 && rp[2] != 2) || rp[1] <= 0 || rp[1] > hd || (rp[1] & 1)) return false;
        if (rq->src[1]->type != GGML_TYPE_I32 || (rq->src[2] && rq->src[2]->type != GGML_TYPE_F32)) return false;
        // libllama hands FLASH_ATTN_EXT an F16 copy of its f32 mask input (llama-graph.cpp: ggml_cast(self_kq_mask, F16), one CPY node per graph, emitted
        // inside the first layer): the stage reads the f32 source instead (0 and -inf are the same numbers in both), and the copy is elided once every one
        // of its consumers is a covered attention stage (decided with the holes, below)
        const struct ggml_tensor * mask_cast = nullptr;
        if (mask && mask->op == GGML_OP_CPY && mask->type == GGML_TYPE_F16 && mask->src[0]->type == GGML_TYPE_F32 && mask->src[0]->op == GGML_OP_NONE &&
            ggml_are_same_shape(mask, mask->src[0]) && ggml_is_contiguous(mask) && ggml_is_contiguous(mask->src[0]) && idx(mask) >= 0) { mask_cast = mask; mask = mask->src[0]; }
        if (mask && (mask->type != GGML_TYPE_F32 && mask->type != GGML_TYPE_F16)) return false;
        if (mask && mask->ne[0] < n_kv) return false;
        if (!mi355_is_vec_f32(top) && !(fa && fa->type == GGML_TYPE_F32 && ggml_is_contiguous(fa))) return false;
        if (!dest_table || cpy_ordinal[(size_t) idx(ck)] < 0 || cpy_ordinal[(size_t) idx(cv)] < 0 || cpy_ordinal[(size_t) idx(ck)] >= MI355_MAX_CPY_DESTS || cpy_ordinal[(size_t) idx(cv)] >= MI355_MAX_CPY_DESTS) return false;

        mi355q_attn * a = new mi355q_attn();
        memset(a, 0, sizeof(*a));
        b.attns.push_back(a);
        a->q = (const float *) qm->data; a->k = (const float *) km->data; a->v = (const float *) vm->data;
        a->q_id = vid(qm); a->k_id = vid(km); a->v_id = vid(vm); a->out_id = vid(top);
        a->pos = (const int32_t *) rq->src[1]->data;
        a->rope.n_dims = rp[1]; a->rope.mode = rp[2]; a->rope.n_ctx_orig = rp[4];
        memcpy(&a->rope.freq_base, rp + 5, 4); memcpy(&a->rope.freq_scale, rp + 6, 4); memcpy(&a->rope.ext_factor, rp + 7, 4);
        memcpy(&a->rope.attn_factor, rp + 8, 4); memcpy(&a->rope.beta_fast, rp + 9, 4); memcpy(&a->rope.beta_slow, rp + 10, 4);
        a->freq_factors = rq->src[2] ? (const float *) rq->src[2]->data : nullptr;
        a->k_cache = kview->data; a->k_nb_pos = (int64_t) kview->nb[1]; a->k_nb_head = (int64_t) kview->nb[2];
        a->v_cache = vview->data;
        if (fa) { if (vview->nb[0] != v_nb0 || vview->ne[0] != hd || vview->ne[1] != n_kv) return false; a->v_nb_dim = (int64_t) v_nb0; a->v_nb_pos = (int64_t) vview->nb[1]; a->v_nb_head = (int64_t) vview->nb[2]; }
        else    { if (vview->nb[0] != 2 || vview->ne[0] != n_kv || vview->ne[1] != hd) return false; a->v_nb_pos = 2; a->v_nb_dim = (int64_t) vview->nb[1]; a->v_nb_head = (int64_t) vview->nb[2]; }
        a->k_dst = (void * const *) (dest_table + cpy_ordinal[(size_t) idx(ck)]);
        a->v_dst = (void * const *) (dest_table + cpy_ordinal[(size_t) idx(cv)]);
        if (ck->src[1]->nb[0] != kv_nb0 || !ggml_is_contiguous(ck->src[1])) return false;       // the K row is stored contiguously
        const struct ggml_tensor * vd = cv->src[1];
        a->v_dst_nb = vd->ne[0] == 1 ? (int64_t) vd->nb[1] : (int64_t) vd->nb[0];
        if (vd->ne[0] != 1 && !ggml_is_contiguous(vd)) return false;
        if (v_quant && (vd->ne[0] == 1 || vd->nb[0] != v_nb0)) return false;                   // (a quantized V row is stored contiguously too)
        a->mask = mask ? mask->data : nullptr; a->mask_f16 = mask && mask->type == GGML_TYPE_F16;
        if (mask_cast) mask_casts.insert(mask_cast);
        a->n_head = (int) n_head; a->n_head_kv = (int) n_head_kv; a->head_dim = (int) hd; a->n_kv = (int) n_kv;
        a->scale = scale;
        a->out = (float *) top->data;
        if (kview->view_src->buffer == nullptr || !mi355_buft_is_ours(kview->view_src->buffer->buft) || !mi355_buft_is_ours(vview->view_src->buffer->buft)) return false;

        const std::string kv_name = kv_mixed ? std::string(ggml_type_name(kvt)) + " / " + ggml_type_name(vvt) : std::string(ggml_type_name(kvt));     // `kv q8_0`, or `kv q8_0 / q4_0` for a mixed cache
        if (getenv("MI355_PLAN_DEBUG"))
            fprintf(stderr, "MI355 plan attn: q %p k %p v %p pos %p | n_head %d n_head_kv %d hd %d n_kv %d | rope n_dims %d mode %d base %g | kv %s | k_cache %p nb_pos %lld nb_head %lld | v_cache %p nb_pos %lld nb_dim %lld nb_head %lld | "
                            "cpy slots k %d v %d (k dst now %p, v dst now %p) v_dst_nb %lld | mask %p f16 %d scale %g | out %p\n",
                    (void *) a->q, (void *) a->k, (void *) a->v, (void *) a->pos, a->n_head, a->n_head_kv, a->head_dim, a->n_kv, a->rope.n_dims, a->rope.mode, a->rope.freq_base, kv_name.c_str(),
                    a->k_cache, (long long) a->k_nb_pos, (long long) a->k_nb_head, a->v_cache, (long long) a->v_nb_pos, (long long) a->v_nb_dim, (long long) a->v_nb_head,
                    cpy_ordinal[(size_t) idx(ck)], cpy_ordinal[(size_t) idx(cv)], ck->data, cv->data, (long long) a->v_dst_nb, a->mask, a->mask_f16, a->scale, (void *) a->out);
        mi355q_stage st; memset(&st, 0, sizeof(st));
        st.kind = MI355Q_STAGE_ATTN; st.attn = a; st.flags = MI355Q_STAGE_NO_PLAIN;
        if (kv_quant) st.flags |= kvt == GGML_TYPE_Q8_0 ? MI355Q_STAGE_KV_Q8_0 : kvt == GGML_TYPE_Q4_0 ? MI355Q_STAGE_KV_Q4_0 : kvt == GGML_TYPE_Q4_1 ? MI355Q_STAGE_KV_Q4_1 :
                                  kvt == GGML_TYPE_Q5_0 ? MI355Q_STAGE_KV_Q5_0 : kvt == GGML_TYPE_Q5_1 ? MI355Q_STAGE_KV_Q5_1 : MI355Q_STAGE_KV_IQ4_NL;
        if (kv_mixed) st.flags |= vvt == GGML_TYPE_F16 ? MI355Q_STAGE_KVV_F16 : vvt == GGML_TYPE_Q8_0 ? MI355Q_STAGE_KVV_Q8_0 : vvt == GGML_TYPE_Q4_0 ? MI355Q_STAGE_KVV_Q4_0 : vvt == GGML_TYPE_Q4_1 ? MI355Q_STAGE_KVV_Q4_1 :
                                  vvt == GGML_TYPE_Q5_0 ? MI355Q_STAGE_KVV_Q5_0 : vvt == GGML_TYPE_Q5_1 ? MI355Q_STAGE_KVV_Q5_1 : MI355Q_STAGE_KVV_IQ4_NL;
        b.stages.push_back(st);
        b.anchor.push_back(idx(fa ? fa : kq));
        b.outs.push_back({ top });
        std::vector<int> mine; std::vector<int> * outer = cur; cur = &mine;
        cover(rq); cover(rk); cover(ck); cover(cv); cover(top);
        if (!fa) { cover(kq); cover(sm); cover(kqv); }
        cur = outer;
        b.nodes.push_back(mine);
        return true;
    }

    // a tensor that may be handed to the plan as an operand vector of n floats
    static bool operand(const struct ggml_tensor * t, int64_t n) {
        return mi355_is_vec_f32(t) && ggml_nelements(t) == n && (t->buffer == nullptr || mi355_buft_is_ours(t->buffer->buft));
    }

    bool match(mi355_plan_build & b) {
        const int n_nodes = g->n_nodes;
        std::vector<char> grouped((size_t) n_nodes, 0);
        std::unordered_map<const struct ggml_tensor *, size_t> folded_x;     // activation tensor X -> the stage that folded its producers into a prologue
        for (int i = 0; i < n_nodes; ++i) {
            const struct ggml_tensor * m0 = g->nodes[i];
            if (grouped[(size_t) i] || !is_mat[(size_t) i]) continue;
            // the other matmuls on the same activation tensor (at most 4 per stage)
            int idxs[4] = { i, -1, -1, -1 }, n = 1;
            for (auto jt = std::upper_bound(mats.begin(), mats.end(), i); jt != mats.end() && n < 4; ++jt) {
                const int j = *jt;
                const struct ggml_tensor * o = g->nodes[j];
                if (!grouped[(size_t) j] && o->src[1] == m0->src[1] && o->src[0]->ne[0] == m0->src[0]->ne[0] &&
                    mi355q_act_type((int) o->src[0]->type) == mi355q_act_type((int) m0->src[0]->type)) idxs[n++] = j;
            }
            mi355q_stage st; memset(&st, 0, sizeof(st));
            st.kind = MI355Q_STAGE_GEMV; st.n_mats = n; st.k = m0->src[0]->ne[0]; st.flags = MI355Q_STAGE_NO_PLAIN;
            std::vector<const struct ggml_tensor *> outs;
            std::vector<int> mine; cur = &mine;
            for (int q = 0; q < n; ++q) {
                const struct ggml_tensor * o = g->nodes[idxs[q]];
                st.mats[q].type = (int) o->src[0]->type; st.mats[q].w = o->src[0]->data; st.mats[q].w_stride = (int64_t) o->src[0]->nb[1];
                st.mats[q].y = (float *) o->data; st.mats[q].y_stride = (int64_t) o->nb[1]; st.mats[q].m = o->src[0]->ne[1];
                st.y_id[q] = vid(o);
                if (!mi355_operand_ok(o->src[0])) return false;
                grouped[(size_t) idxs[q]] = 1; covered[(size_t) idxs[q]] = 1; mine.push_back(idxs[q]);
                outs.push_back(o);
            }
            // gate | up feeding MUL(UNARY(gate), up): the producer publishes the product (one vector for ffn_down to gather instead of two)
            if (n == 2 && st.mats[0].type == st.mats[1].type && st.mats[0].m == st.mats[1].m) {
                const struct ggml_tensor * o0 = g->nodes[idxs[0]], * o1 = g->nodes[idxs[1]];
                for (int j = idxs[1] + 1; j < n_nodes && j <= idxs[1] + 8; ++j) {
                    const struct ggml_tensor * M = g->nodes[j];
                    if (M->op != GGML_OP_MUL || covered[(size_t) j]) continue;
                    const struct ggml_tensor * U = M->src[0]->op == GGML_OP_UNARY ? M->src[0] : (M->src[1]->op == GGML_OP_UNARY ? M->src[1] : nullptr);
                    if (!U) continue;
                    const struct ggml_tensor * B = U == M->src[0] ? M->src[1] : M->src[0];
                    const struct ggml_tensor * A = U->src[0];
                    const int uop = mi355_unary_code(ggml_get_unary_op(U));
                    if (!((A == o0 && B == o1) || (A == o1 && B == o0)) || (uop != MI355Q_UNARY_SILU && uop != MI355Q_UNARY_RELU && uop != MI355Q_UNARY_SIGMOID)) continue;
                    if (!single_use(o0) || !single_use(o1) || !single_use(U) || !mi355_is_vec_f32(M) || ggml_nelements(M) != st.mats[0].m || idx(U) < 0 || covered[(size_t) idx(U)]) break;
                    if (A == o1) { std::swap(st.mats[0], st.mats[1]); }                  // mats[0] is the matrix under the unary
                    st.y_kind = MI355Q_Y_UNARY_MUL; st.y_unary = uop;
                    st.mats[0].y = (float *) M->data; st.y_id[0] = vid(M); st.y_id[1] = 0;
                    outs.clear(); outs.push_back(M);
                    cover(U); cover(M);
                    break;
                }
            }
            const int64_t k = st.k;
            const struct ggml_tensor * X = m0->src[1];
            st.x_kind = MI355Q_X_PLAIN; st.x = (const float *) X->data; st.x_id = vid(X);
            bool folded = false;
            {   // a second group on the same activations (matrices of the other activation format, e.g. a Q5_K attn_v beside IQ4_NL wq / wk): the same
                // prologue again -- its stage gathers and quantizes the same operands in its own format; the sum was published by the first
                auto fx = folded_x.find(X);
                if (fx != folded_x.end()) {
                    const mi355q_stage & f = b.stages[fx->second];
                    st.x_kind = f.x_kind; st.x_unary = f.x_unary; st.x = f.x; st.x1 = f.x1; st.norm_w = f.norm_w; st.eps = f.eps; st.x_id = f.x_id; st.x1_id = f.x1_id;
                    folded = true;
                }
            }
            if (!folded && X->op == GGML_OP_MUL && idx(X) >= 0 && !covered[(size_t) idx(X)]) {
                const struct ggml_tensor * p0 = X->src[0], * p1 = X->src[1];
                const struct ggml_tensor * N = p0->op == GGML_OP_RMS_NORM ? p0 : (p1->op == GGML_OP_RMS_NORM ? p1 : nullptr);
                const struct ggml_tensor * U = p0->op == GGML_OP_UNARY ? p0 : (p1->op == GGML_OP_UNARY ? p1 : nullptr);
                if (N && idx(N) >= 0 && !covered[(size_t) idx(N)] && single_use(N)) {
                    const struct ggml_tensor * w = N == p0 ? p1 : p0;
                    const struct ggml_tensor * T = N->src[0];
                    if (idx(w) < 0 && operand(w, k) && operand(T, k) && ggml_nelements(N) == k) {      // w: a weight (not computed in this graph)
                        st.x_kind = MI355Q_X_NORM; st.norm_w = (const float *) w->data; memcpy(&st.eps, N->op_params, 4);
                        const struct ggml_tensor * a0 = T->op == GGML_OP_ADD ? through_rows(T->src[0]) : nullptr, * a1 = T->op == GGML_OP_ADD ? through_rows(T->src[1]) : nullptr;
                        if (T->op == GGML_OP_ADD && idx(T) >= 0 && !covered[(size_t) idx(T)] && operand(a0, k) && operand(a1, k)) {
                            st.x = (const float *) a0->data; st.x1 = (const float *) a1->data; st.sum_out = (float *) T->data;
                            st.x_id = vid(a0); st.x1_id = vid(a1); st.sum_id = vid(T);
                            if (a0 != T->src[0]) cover(T->src[0]);
                            if (a1 != T->src[1]) cover(T->src[1]);
                            cover(T); outs.push_back(T);
                        } else { st.x = (const float *) T->data; st.x_id = vid(T); }
                        if (needs_x_out(X, g->nodes[idxs[n - 1]])) { st.x_out = (float *) X->data; }
                        cover(N); cover(X); folded = true;
                    }
                } else if (U && idx(U) >= 0 && !covered[(size_t) idx(U)]) {
                    const int uop = mi355_unary_code(ggml_get_unary_op(U));
                    const struct ggml_tensor * B = U == p0 ? p1 : p0;
                    if ((uop == MI355Q_UNARY_SILU || uop == MI355Q_UNARY_RELU || uop == MI355Q_UNARY_SIGMOID) && operand(U->src[0], k) && operand(B, k) && single_use(U)) {
                        st.x_kind = MI355Q_X_UNARY_MUL; st.x_unary = uop; st.x = (const float *) U->src[0]->data; st.x1 = (const float *) B->data;
                        st.x_id = vid(U->src[0]); st.x1_id = vid(B);
                        if (needs_x_out(X, g->nodes[idxs[n - 1]])) st.x_out = (float *) X->data;
                        cover(U); cover(X); folded = true;
                    }
                }
            }
            if (!folded) {
                if (!operand(X, k)) return false;
                // the attention block's output?  (CONT of the permuted K.Q.V product, or the reshaped FLASH_ATTN_EXT node)
                const struct ggml_tensor * top = X->op == GGML_OP_CONT ? X : mi355_skip_views(X);
                if (top && idx(top) >= 0 && !covered[(size_t) idx(top)] && (top->op == GGML_OP_CONT || top->op == GGML_OP_FLASH_ATTN_EXT)) {
                    std::vector<int> * mine_p = cur;
                    (void) match_attn(top, b);                    // (no match: the attention nodes stay uncovered and this stage falls behind the hole they leave)
                    cur = mine_p;
                }
            }
            cur = nullptr;
            if (folded && folded_x.find(X) == folded_x.end()) folded_x[X] = b.stages.size();
            b.stages.push_back(st);
            b.anchor.push_back(i);
            b.outs.push_back(outs);
            b.nodes.push_back(mine);
        }
        return !b.stages.empty();
    }
};

// Build (or decline) the plan of a graph.  On success `e` holds the plan and the prefix / suffix node lists.
static bool mi355_plan_compile(mi355_backend_ctx * ctx, struct ggml_cgraph * cgraph, mi355_plan_entry & e) {
    static const bool dbg = getenv("MI355_PLAN_DEBUG") != nullptr;
#define PLAN_DECLINE(why) do { if (dbg) fprintf(stderr, "MI355 plan declined (%d nodes): %s\n", cgraph->n_nodes, why); return false; } while (0)
    if (cgraph->n_nodes < 8) return false;
    // one token only: every quantized matmul must have a single activation row (cheap pre-check before any matching)
    int n_mats = 0;
    for (int i = 0; i < cgraph->n_nodes; ++i) {
        const struct ggml_tensor * n = cgraph->nodes[i];
        if (n->op == GGML_OP_MUL_MAT_ID) PLAN_DECLINE("MUL_MAT_ID");
        if (n->op == GGML_OP_MUL_MAT && mi355_is_quant(n->src[0]->type)) { if (!mi355_plan_mat(n)) PLAN_DECLINE("a quantized MUL_MAT with more than one activation row / no streaming kernel"); ++n_mats; }
    }
    if (n_mats < 2) return false;
    static const bool laps = getenv("MI355_TIMING") != nullptr;
    const auto t_m0 = std::chrono::steady_clock::now();
    mi355_plan_build b;
    mi355_plan_matcher mt(cgraph, ctx->dest_table);
    if (!mt.match(b)) PLAN_DECLINE("a node pattern the matcher does not know");
    const auto t_m1 = std::chrono::steady_clock::now();
    // order the stages by their anchor nodes (a topological order: every stage's operands are produced by nodes before its anchor)
    std::vector<int> order(b.stages.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int) i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return b.anchor[(size_t) x] < b.anchor[(size_t) y]; });
    // Uncovered compute nodes may only form a prefix and a suffix of the node list.  A scheduler split can end in the middle of a layer (its tail
    // then matches no stage, or only part of one): every stage that reaches past the first such hole is dropped and its nodes join the suffix,
    // until the kept stages form one gap-free block.
    std::vector<char> keep(b.stages.size(), 1);
    for (;;) {
        for (const struct ggml_tensor * mc : mt.mask_casts) {     // a mask copy is elided only while every node that reads it is a covered stage
            bool all = true;
            for (int i = 0; i < cgraph->n_nodes && all; ++i)
                for (int sI = 0; sI < GGML_MAX_SRC && all && cgraph->nodes[i] != mc; ++sI)     // (a ggml_cast node names itself as src[1])
                    for (const struct ggml_tensor * t = cgraph->nodes[i]->src[sI]; t; t = t->view_src) if (t == mc && !mt.covered[(size_t) i]) { all = false; break; }
            mt.covered[(size_t) mt.idx(mc)] = all ? 1 : 0;
        }
        int first_cov = -1;
        for (int i = 0; i < cgraph->n_nodes && first_cov < 0; ++i) if (mt.covered[(size_t) i]) first_cov = i;
        int hole = -1;
        for (int i = first_cov; i >= 0 && i < cgraph->n_nodes; ++i) {
            const struct ggml_tensor * n = cgraph->nodes[i];
            if (!mt.covered[(size_t) i] && !mi355_is_view_op(n) && !ggml_is_empty(n)) { hole = i; break; }
        }
        bool dropped = false;
        if (hole >= 0 && dbg) fprintf(stderr, "MI355 plan: node %d (%s, %s) is covered by no stage: the stages that reach past it are dropped\n", hole, ggml_op_desc(cgraph->nodes[hole]), cgraph->nodes[hole]->name);
        if (hole >= 0) for (size_t si = 0; si < b.stages.size(); ++si) {
            if (!keep[si]) continue;
            int mx = -1; for (int ni : b.nodes[si]) mx = std::max(mx, ni);
            if (mx > hole) { keep[si] = 0; dropped = true; for (int ni : b.nodes[si]) mt.covered[(size_t) ni] = 0; }
        }
        if (!dropped) break;
    }
    {
        mi355_plan_build kb;
        for (size_t si = 0; si < b.stages.size(); ++si) if (keep[si]) { kb.stages.push_back(b.stages[si]); kb.anchor.push_back(b.anchor[si]); kb.outs.push_back(b.outs[si]); kb.nodes.push_back(b.nodes[si]); }
        kb.attns.swap(b.attns);                                  // (ownership of every attention descriptor moves along; unused ones are freed with kb)
        b.stages.swap(kb.stages); b.anchor.swap(kb.anchor); b.outs.swap(kb.outs); b.nodes.swap(kb.nodes); b.attns.swap(kb.attns);
    }
    int n_gemv = 0; for (auto & st : b.stages) n_gemv += st.kind == MI355Q_STAGE_GEMV;
    if (n_gemv < 2) PLAN_DECLINE("fewer than two matmul stages form a gap-free block");
    order.resize(b.stages.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int) i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return b.anchor[(size_t) x] < b.anchor[(size_t) y]; });
    int first_cov = -1, last_cov = -1;
    for (int i = 0; i < cgraph->n_nodes; ++i) if (mt.covered[(size_t) i]) { if (first_cov < 0) first_cov = i; last_cov = i; }
    e.pre.clear(); e.post.clear();
    for (int i = 0; i < cgraph->n_nodes; ++i) {
        const struct ggml_tensor * n = cgraph->nodes[i];
        if (mt.covered[(size_t) i] || mi355_is_view_op(n) || ggml_is_empty(n)) continue;
        if (i < first_cov) e.pre.push_back(i); else if (i > last_cov) e.post.push_back(i);
        else { if (dbg) fprintf(stderr, "MI355 plan: node %d (%s) between covered nodes is not part of any stage\n", i, ggml_op_desc(n)); PLAN_DECLINE("uncovered node inside the plan"); }
    }
    // operands computed by PREFIX nodes are plain vectors for the plan: drop their value ids
    auto plain_if_uncovered = [&](int64_t & id) { if (id > 0 && !mt.covered[(size_t) (id - 1)]) id = 0; };
    for (auto & st : b.stages) {
        plain_if_uncovered(st.x_id); plain_if_uncovered(st.x1_id);
        if (st.kind == MI355Q_STAGE_ATTN) { mi355q_attn * a = const_cast<mi355q_attn *>(st.attn); plain_if_uncovered(a->q_id); plain_if_uncovered(a->k_id); plain_if_uncovered(a->v_id); }
    }
    // plain stores: graph outputs, whatever the suffix nodes read from the plan, and tensors nobody in THIS graph consumes (the graph is a
    // scheduler split and the consumer lives in another one)
    std::unordered_map<const struct ggml_tensor *, int> n_uses;
    for (int i = 0; i < cgraph->n_nodes; ++i) for (int s = 0; s < GGML_MAX_SRC; ++s)
        for (const struct ggml_tensor * src = cgraph->nodes[i]->src[s]; src; src = src->view_src) ++n_uses[src];
    auto needs_plain = [&](const struct ggml_tensor * t) {
        if (t->flags & GGML_TENSOR_FLAG_OUTPUT) return true;
        if (n_uses.find(t) == n_uses.end()) return true;
        for (int j : e.post) for (int s = 0; s < GGML_MAX_SRC; ++s) {
            const struct ggml_tensor * src = cgraph->nodes[j]->src[s];
            for (; src; src = src->view_src) if (src == t) return true;
        }
        return false;
    };
    for (size_t i = 0; i < b.stages.size(); ++i) for (const struct ggml_tensor * t : b.outs[i]) if (needs_plain(t)) b.stages[i].flags &= ~MI355Q_STAGE_NO_PLAIN;
    // operands produced inside the graph must come from the plan itself (an earlier stage) or from the prefix
    // (mi355q_plan_create resolves them by address; a producer that is neither would be read before it is written)
    std::vector<mi355q_stage> sorted;
    for (int i : order) sorted.push_back(b.stages[(size_t) i]);
    mi355q_plan * plan = nullptr;
    if (laps) fprintf(stderr, "MI355 plan compile: match %.0f us, order + holes %.0f us\n", std::chrono::duration<double, std::micro>(t_m1 - t_m0).count(),
                      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_m1).count());
    if (mi355q_plan_create(&plan, sorted.data(), (int) sorted.size(), 0) != MI355Q_OK) {
        if (dbg) fprintf(stderr, "MI355 plan_create: %s\n", mi355q_last_error());
        PLAN_DECLINE("plan_create failed");
    }
    e.plan = plan; e.n_stages = (int) sorted.size();
    if (dbg) {
        fprintf(stderr, "MI355 plan: %d stages (%d launch stages), %zu prefix + %zu suffix nodes of %d\n", e.n_stages, mi355q_plan_launch_stages(plan), e.pre.size(), e.post.size(), cgraph->n_nodes);
        for (size_t i = 0; i < sorted.size() && i < 16; ++i) {
            const mi355q_stage & st = sorted[i];
            if (st.kind == MI355Q_STAGE_ATTN) fprintf(stderr, "  stage %2zu ATTN n_kv %d heads %d/%d flags %x\n", i, st.attn->n_kv, st.attn->n_head, st.attn->n_head_kv, st.flags);
            else fprintf(stderr, "  stage %2zu GEMV k %lld mats %d (m0 %lld type %d) x_kind %d x1 %d norm_w %d sum_out %d y_kind %d flags %x\n", i, (long long) st.k, st.n_mats,
                         (long long) st.mats[0].m, st.mats[0].type, st.x_kind, st.x1 != nullptr, st.norm_w != nullptr, st.sum_out != nullptr, st.y_kind, st.flags);
        }
    }
    return true;
}
