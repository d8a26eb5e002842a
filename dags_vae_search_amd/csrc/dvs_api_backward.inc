// Backward + optimizer entry points (included by dvs_api.hip).

// Argument blocks of the backward phases, from the call context (dvs_api.hip: Step) plus what varies.  in: activation slot
// of the sublayer's input; norm: LayerNorm of the producer of `in` (null: an embedding), whose weight gradients the phase
// also owns; gpre: d(pre-sum) of this sublayer; site0: first of its two consecutive dropout sites.
static AttnBwdArgs attn_bwd_args(const Step& c, const DvsAttnP& ap, int block, int in, const DvsNormP* norm, const float* kv,
                                 const float* gpre, int site0) {
    AttnBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.wimg = wimg_attn(c, block);
    a.dims = c.d;
    a.rec = c.rec;
    a.xin = c.ws + c.W.act[in];
    a.ln = ln_of(c, in, norm);
    a.kv = kv;
    a.in_w = c.P + ap.in_w;
    a.in_b = c.P + ap.in_b;
    a.out_w = c.P + ap.out_w;
    a.out_b = c.P + ap.out_b;
    a.gpre = gpre;
    a.gq = c.ws + c.W.gq;
    a.gk = c.ws + c.W.gk;
    a.gv = c.ws + c.W.gv;
    a.site_prob = site0;
    a.site_post = site0 + 1;
    a.slab = c.ws + c.W.slabs;
    a.P = c.L.total;
    a.o_out_w = ap.out_w;
    a.o_out_b = ap.out_b;
    a.qkv = c.wide ? c.ws + c.W.qkv[block] : nullptr;      // as the forward parked them
    return a;
}

// the q, k, v in-projections of attention block `block` behind k_attn_bwd: gy = (gq, gk, gv), d input = gres + ... -> gout
static ProjBwdArgs proj_bwd_args(const Step& c, const DvsAttnP& ap, int block, int in, const DvsNormP* norm, const float* gres,
                                 float* gout) {
    ProjBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.dims = c.d;
    a.xin = c.ws + c.W.act[in];
    a.ln = ln_of(c, in, norm);
    a.w = c.P + ap.in_w;
    a.wimg = (const dvs_bf16*)wimg_attn(c, block) + DvsAttnImg::WinT;
    a.gy[0] = c.ws + c.W.gq;
    a.gy[1] = c.ws + c.W.gk;
    a.gy[2] = c.ws + c.W.gv;
    a.gres = gres;
    a.gout = gout;
    a.slot_order = c.wide ? 0 : 1;      // the wide attention kernels keep q/k/v in parameter order; the one-tile ones in head-aligned slot order
    a.slab = c.ws + c.W.slabs;
    a.P = c.L.total;
    a.o_w = ap.in_w;
    a.o_b = ap.in_b;
    a.o_ln_g = norm ? norm->w : -1;
    a.o_ln_b = norm ? norm->b : -1;
    return a;
}

static FfnBwdArgs ffn_bwd_args(const Step& c, const DvsFfnP& fp, int block, int in, const DvsNormP& norm, const float* gpre,
                               float* gout, int site0) {
    FfnBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.dims = c.d;
    a.xin = c.ws + c.W.act[in];
    a.ln = ln_of(c, in, &norm);
    a.l1_w = c.P + fp.l1_w;
    a.l1_b = c.P + fp.l1_b;
    a.l2_w = c.P + fp.l2_w;
    a.l2_b = c.P + fp.l2_b;
    a.wimg = wimg_ffn(c, block);
    a.gpre = gpre;
    a.gout = gout;
    a.site_hidden = site0;
    a.site_post = site0 + 1;
    a.slab = c.ws + c.W.slabs;
    a.P = c.L.total;
    a.o_l1_w = fp.l1_w;
    a.o_l1_b = fp.l1_b;
    a.o_l2_w = fp.l2_w;
    a.o_l2_b = fp.l2_b;
    a.o_ln_g = norm.w;
    a.o_ln_b = norm.b;
    a.o_own_g = -1;
    a.o_own_b = -1;
    return a;
}

extern "C" int dvs_loss_backward(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                                 int64_t n_params, void* workspace, size_t workspace_bytes, const float* gcoef,
                                 float* grads, void* stream) {
    return dvs_loss_backward_sq(s, records, records_bytes, params, n_params, workspace, workspace_bytes, gcoef, grads, nullptr,
                                stream);
}

extern "C" int dvs_loss_backward_sq(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                                    int64_t n_params, void* workspace, size_t workspace_bytes, const float* gcoef,
                                    float* grads, float* clip_scratch, void* stream) {
    return dvs_loss_backward_emit(s, records, records_bytes, params, n_params, workspace, workspace_bytes, gcoef, grads,
                                  clip_scratch, nullptr, nullptr, nullptr, 0u, stream);      // no losses: the plain loss-head backward
}

extern "C" int dvs_loss_backward_emit(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                                      int64_t n_params, void* workspace, size_t workspace_bytes, const float* gcoef,
                                      float* grads, float* clip_scratch, int32_t* status, float* losses, void* host_tail,
                                      uint32_t host_seq, void* stream) {
    if (int e = check_shape(s)) return e;
    if (!records || !params || !workspace || !gcoef || !grads) return fail(10, "dvs_loss_backward: null pointer");
    const Step c = make_step(s, records, params, workspace, stream);
    if (int e = check_buffers(c, "dvs_loss_backward", records_bytes, n_params, workspace_bytes)) return e;
    const bool emit_loss = losses != nullptr;      // behind dvs_loss_forward_defer: the loss head runs once, here
    if (emit_loss && c.wide) return fail(13, "dvs_loss_backward_emit: one-tile path only (n_tokens, n_classes <= 16)");
    if (clip_scratch && 2 + dvs_sq_parts(c.L.total) > DVS_CLIP_SCRATCH_FLOATS)
        return fail(14, "dvs_loss_backward_sq: clip_scratch (DVS_CLIP_SCRATCH_FLOATS) is too small for this parameter count");
    call_begin();
    const DvsLayout& L = c.L;
    const DvsWorkspace& W = c.W;
    float* ws = c.ws;
    dvs_stream_t st = c.st;
    const bool wide = c.wide;
    const int grid = c.slabs;      // workgroups of every backward kernel = slabs written and reduced this step
    const int nw = c.nw;
    // One-tile path: the stack's phases are chained into launches of up to DVS_STACK_PHASES (k_bwd_stack); the wide path
    // and DVS_SPLIT_STACK=1 launch every phase on its own.
    const bool chain = !wide && !split_stack();
    // wide path: the token-local phases BETWEEN two attention launches (a layer's q / k / v projections and the FFN of the layer
    // below) still travel as one chained launch; k_attn_bwd_w flushes what has gathered
    const bool chain_local = wide && !split_stack();
    BwdStackArgs stack;
    memset(&stack, 0, sizeof(stack));
    int stack_tag = 0;
    auto flush_stack = [&]() {
        if (stack.nphase > 0) dvs_launch_bwd_stack(stack, stack_tag, grid, nw, st);
        stack.nphase = 0;
        stack.has_latent = 0;
    };
    auto next_phase = [&](int kind) -> BwdPhase& {
        if (stack.nphase == DVS_STACK_PHASES) flush_stack();
        BwdPhase& ph = stack.ph[stack.nphase++];
        ph.kind = kind;
        return ph;
    };
    auto launch_ffn_bwd = [&](const FfnBwdArgs& f) {
        if (chain || chain_local) next_phase(DVS_PH_FFN).u.f = f;
        else dvs_launch_ffn_bwd(f, grid, nw, st);
    };
    auto launch_attn_bwd = [&](const AttnBwdArgs& a) {
        if (chain) {
            next_phase(DVS_PH_ATTN).u.a = a;
        } else if (wide) {
            flush_stack();
            dvs_launch_attn_bwd_w(a, grid, st);
        } else {
            dvs_launch_attn_bwd(a, grid, nw, st);
        }
    };
    auto launch_proj_bwd = [&](const ProjBwdArgs& a) {      // all three projections
        if (chain || chain_local) next_phase(DVS_PH_PROJ1 + 2).u.p = a;
        else dvs_launch_proj_bwd(a, 3, grid, nw, st);
    };

    // ---- loss head (+ last decoder LayerNorm) -------------------------------------------------------------------
    float* cur = ws + W.gA;
    float* oth = ws + W.gB;
    {
        LossArgs la = loss_args(c);
        la.gcoef = gcoef;
        la.gout = cur;
        la.slab = ws + W.slabs;
        la.P = L.total;
        la.o_node0_w = L.node0_w;
        la.o_node0_b = L.node0_b;
        la.o_node2_w = L.node2_w;
        la.o_node2_b = L.node2_b;
        la.o_edge0_w = L.edge0_w;
        la.o_edge0_b = L.edge0_b;
        la.o_edge2_w = L.edge2_w;
        la.o_edge2_b = L.edge2_b;
        la.o_ln_g = L.dec[DVS_LAYERS - 1].n3.w;
        la.o_ln_b = L.dec[DVS_LAYERS - 1].n3.b;
        if (wide) dvs_launch_loss_bwd_w(la, grid, st);
        else dvs_launch_loss_bwd(la, grid, emit_loss, st);
        // the per-DAG losses are complete (KL: the latent block of the forward; reconstruction: the launch above)
        if (emit_loss) dvs_launch_finalize(finalize_args(c, status, losses, host_tail, host_seq), st);
    }
    const int dec_in = c.d.drop.on ? 7 : 0;
    // ---- decoder, last layer first --------------------------------------------------------------------------------
    for (int i = DVS_LAYERS - 1; i >= 0; --i) {
        const auto& pl = L.dec[i];
        const int s0 = slot_dec(i, 0), s1 = slot_dec(i, 1);
        // FFN sublayer: input = LN2(pre s1)
        launch_ffn_bwd(ffn_bwd_args(c, pl.ff, blk_dec_ffn(i), s1, pl.n2, cur, oth, site_dec(i, 4)));
        std::swap(cur, oth);
        // cross-attention sublayer: query input = LN1(pre s0), keys/values = memory
        launch_attn_bwd(attn_bwd_args(c, pl.ca, blk_dec_cross(i), s0, &pl.n1, ws + W.mem, cur, site_dec(i, 2)));
        // q projection (input LN1(pre s0), residual gradient, LayerNorm backward) and k / v projections (input = the decoder
        // memory, gradient accumulated over the layers into gmem) as ONE split phase: a phase's fixed cost (tail + cold
        // start, ~20 k cycles) is as large as one DAG round of either
        ProjBwdArgs pq = proj_bwd_args(c, pl.ca, blk_dec_cross(i), s0, &pl.n1, cur, oth);
        pq.xin2 = ws + W.mem;
        pq.gout2 = ws + W.gmem;
        pq.accumulate_out2 = i != DVS_LAYERS - 1;
        launch_proj_bwd(pq);
        std::swap(cur, oth);
        // self-attention sublayer: input = LN3 of the previous layer (or the decoder embedding)
        const int sp = i > 0 ? slot_dec(i - 1, 2) : dec_in;
        const DvsNormP* np = i > 0 ? &L.dec[i - 1].n3 : nullptr;
        launch_attn_bwd(attn_bwd_args(c, pl.sa, blk_dec_self(i), sp, np, nullptr, cur, site_dec(i, 0)));
        launch_proj_bwd(proj_bwd_args(c, pl.sa, blk_dec_self(i), sp, np, cur, oth));
        std::swap(cur, oth);
    }
    flush_stack();
    stack_tag = 1;
    float* gdec_emb = cur;   // d(decoder input embedding)
    float* freebuf = oth;

    // ---- latent block ----------------------------------------------------------------------------------------------
    // inside the encoder chain when there is one (k_bwd_stack<1>, ahead of the chain's first phase): k_fc_dw then follows
    // the chain's LAST launch.  Decided HERE: flush_stack() clears has_latent, also when it runs mid-chain.
    const bool fc_deferred = latent_in_chain(chain, nw);
    FcDwArgs fcdw;
    {
        LatentBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dims = c.d;
        a.gmem = ws + W.gmem;
        a.mu = ws + W.mu;
        a.logvar = ws + W.logvar;
        a.epsv = ws + W.epsv;
        a.limg = ws + W.limg;
        a.gcoef = gcoef;
        a.gz = ws + W.gz;
        a.genc = ws + W.genc;
        if (fc_deferred) {
            stack.has_latent = 1;
            stack.lat = a;
        } else {
            dvs_launch_latent_bwd(a, st);
        }
        FcDwArgs& f = fcdw;
        memset(&f, 0, sizeof(f));
        f.dims = c.d;
        f.gz = ws + W.gz;
        f.xenc = ws + W.enc_out;
        f.gmem = ws + W.gmem;
        f.z = ws + W.z;
        f.fcpart = ws + W.fcpart;
        f.P = L.total;
        f.o_fc1_w = L.fc1_w;
        f.o_fc1_b = L.fc1_b;
        f.o_fc2_w = L.fc2_w;
        f.o_fc2_b = L.fc2_b;
        f.o_fc3_w = L.fc3_w;
        f.o_fc3_b = L.fc3_b;
        if (!fc_deferred) dvs_launch_fc_dw(f, st);          // chained: behind the encoder chain, which produces gz
    }
    // ---- encoder ---------------------------------------------------------------------------------------------------
    cur = ws + W.genc;
    oth = freebuf;
    for (int i = DVS_LAYERS - 1; i >= 0; --i) {
        const auto& pl = L.enc[i];
        const int s0 = slot_enc(i, 0), s1 = slot_enc(i, 1);
        FfnBwdArgs f = ffn_bwd_args(c, pl.ff, blk_enc_ffn(i), s0, pl.n1, cur, oth, site_enc(i, 2));
        if (i == DVS_LAYERS - 1) {   // d enc_out is w.r.t. LN2(pre s1): pull back through it first
            f.own_pre = ws + W.act[s1];
            f.own = ln_of(c, s1, &pl.n2);
            f.o_own_g = pl.n2.w;
            f.o_own_b = pl.n2.b;
        }
        launch_ffn_bwd(f);
        std::swap(cur, oth);
        const int sp = i > 0 ? slot_enc(i - 1, 1) : 0;
        const DvsNormP* np = i > 0 ? &L.enc[i - 1].n2 : nullptr;
        launch_attn_bwd(attn_bwd_args(c, pl.sa, blk_enc_attn(i), sp, np, nullptr, cur, site_enc(i, 0)));
        launch_proj_bwd(proj_bwd_args(c, pl.sa, blk_enc_attn(i), sp, np, cur, oth));
        std::swap(cur, oth);
    }
    flush_stack();
    if (fc_deferred) dvs_launch_fc_dw(fcdw, st);
    // ---- embeddings (encoder-side and decoder-side gradients; same weights) --------------------------------------------
    {
        EmbedArgs e = embed_args(c, 0);
        e.gout = cur;
        e.slab = ws + W.slabs;
        e.P = L.total;
        e.oW1 = L.W1;
        e.oW2 = L.W2;
        e.olab_w = L.lab_w;
        e.olab_b = L.lab_b;
        if (wide) dvs_launch_embed_bwd_w(e, gdec_emb, 2, grid, st);
        else dvs_launch_embed_bwd(e, gdec_emb, 2, grid, nw, st);
    }
    ReduceArgs r;
    r.slab = ws + W.slabs;
    r.fcpart = ws + W.fcpart;
    r.grads = grads;
    r.P = L.total;
    r.nslab = grid;
    r.fc_lo1 = L.fc1_w;
    r.fc_hi1 = L.dec[0].sa.in_w;     // fc1.weight .. fc2.bias are contiguous, the decoder follows
    r.fc_lo2 = L.fc3_w;
    r.fc_hi2 = L.total;
    r.sqpart = clip_scratch ? clip_scratch + 2 : nullptr;
    dvs_launch_reduce_slabs(r, st);
    return call_end("dvs_loss_backward");
}

extern "C" int dvs_clip_adam(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float lr,
                             float beta1, float beta2, float adam_eps, int64_t step, float max_norm, float* scratch,
                             const float* guard, void* stream) {
    if (n <= 0 || !params || !grads || !exp_avg || !exp_avg_sq || !scratch) return fail(10, "dvs_clip_adam: bad argument");
    if (step < 1) return fail(12, "dvs_clip_adam: step is 1-based");
    call_begin();
    dvs_launch_clip_adam(n, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, adam_eps, step, max_norm, scratch, guard, false,
                         (dvs_stream_t)stream);
    return call_end("dvs_clip_adam");
}

extern "C" int dvs_clip_adam_from_partials(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float lr,
                                           float beta1, float beta2, float adam_eps, int64_t step, float max_norm,
                                           float* scratch, const float* guard, void* stream) {
    if (n <= 0 || !params || !grads || !exp_avg || !exp_avg_sq || !scratch) return fail(10, "dvs_clip_adam_from_partials: bad argument");
    if (step < 1) return fail(12, "dvs_clip_adam_from_partials: step is 1-based");
    if (2 + dvs_sq_parts(n) > DVS_CLIP_SCRATCH_FLOATS) return fail(14, "dvs_clip_adam_from_partials: more partials than the scratch holds");
    call_begin();
    dvs_launch_clip_adam(n, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, adam_eps, step, max_norm, scratch, guard, true,
                         (dvs_stream_t)stream);
    return call_end("dvs_clip_adam_from_partials");
}
