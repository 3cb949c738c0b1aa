// Builder: the linear-attention modules of imagen-pytorch (LinearAttentionTransformerBlock, LinearCrossAttention) on the
// NHWC token rows.  ChanLayerNorm over the channels of an NCHW map is the gain-only row LayerNorm here, and the 1 x 1
// convs are token GEMMs; the per-step attention itself is kernels_linattn.hip.
namespace kd {

// x1 = LN(proj) g_out + x, then the feed-forward (LayerNorm -> GEMM -> GELU -> LayerNorm -> GEMM) with its residual:
// the tail of TransformerBlock::forward, shared by the ChanFeedForward of the linear block (same keys, weights
// [hidden][dim] either way)
T Builder::feed_forward_tail(const T& x, const T& proj, const std::string& g_out, const std::string& f, const T* dst) {
  const int dim = x.C, hidden = dim * cfg.ff_mult_x2 / 2;
  T h0;
  const bool gelu_late = linear_is_x3(proj, hidden);
  T x1 = layernorm(proj, P(g_out, dim), nullptr, &x, ACT_NONE, P(f + ".0.g", dim), &h0, false, gelu_late ? 2 : 0);
  T h1 = linear(h0, P(f + ".1.weight", (int64_t)hidden * dim), nullptr, hidden, gelu_late ? ACT_NONE : ACT_GELU);
  free(h0);
  T h2 = layernorm(h1, P(f + ".3.g", hidden), nullptr, nullptr, gelu_late ? ACT_GELU : ACT_NONE, nullptr, nullptr, false,
                   linear_is_x3(h1, dim, &x1, dst) ? 1 : 0);
  free(h1);
  T y = linear(h2, P(f + ".4.weight", (int64_t)dim * hidden), nullptr, dim, ACT_NONE, &x1, dst);
  free(h2);
  free(x1);
  return y;
}

// LinearAttentionTransformerBlock (depth 1): x = attn(x, ctx) + x ; x = ff(x) + x.  Launches: LayerNorm, ONE GEMM to
// q | k | v (N = 3 inner, weights stacked at plan build), the depthwise 3 x 3 conv of all three (+ k's softmax partials),
// the context reduction (+ its combine, which adds the context tokens), the apply (SiLU), to_out's GEMM, then the
// feed-forward tail.  `dst`: the last GEMM writes there (a skip slot).
T Builder::linear_attn_block(const T& x, const std::string& pre, const T* ctx, const T* dst) {
  const int H = cfg.attn_heads, D = cfg.attn_dim_head, inner = H * D, dim = x.C, C3 = 3 * inner;
  const std::string a = pre + ".layers.0.0", f = pre + ".layers.0.1";
  T xn = layernorm(x, P(a + ".norm.g", dim), nullptr, nullptr, ACT_NONE, nullptr, nullptr, false,
                   linear_is_x3(x, C3) ? 1 : 0);
  const float* w1[3] = {raw(a + ".to_q.1.weight", (int64_t)inner * dim), raw(a + ".to_k.1.weight", (int64_t)inner * dim),
                        raw(a + ".to_v.1.weight", (int64_t)inner * dim)};
  const float* wqkv = cached("linattn_qkv:" + a, (size_t)C3 * dim, [&](float* dst_) {
    for (int i = 0; i < 3; ++i)
      KD_HIP_THROW(hipMemcpyAsync(dst_ + (size_t)i * inner * dim, w1[i], (size_t)inner * dim * sizeof(float),
                                  hipMemcpyDeviceToDevice, 0));
  });
  const float* w2[3] = {raw(a + ".to_q.2.weight", (int64_t)inner * 9), raw(a + ".to_k.2.weight", (int64_t)inner * 9),
                        raw(a + ".to_v.2.weight", (int64_t)inner * 9)};
  const float* wdw = cached("linattn_dw:" + a, (size_t)9 * C3,
                            [&](float* dst_) { KD_THROW_IF(launch_linattn_pack_dw(w2[0], w2[1], w2[2], dst_, inner, 0)); });
  T qkv = linear(xn, wqkv, nullptr, C3);
  free(xn);
  // context tokens: to_context(c) = Linear(LayerNorm(c)) [B, m, 2 inner], a function of c alone (cond region)
  T ckv;
  const bool has_ctx = ctx != nullptr;
  if (has_ctx) {
    auto ph = cond_scope();
    T cn = layernorm(*ctx, P(a + ".to_context.0.weight", ctx->C), P(a + ".to_context.0.bias", ctx->C));
    ckv = linear(cn, P(a + ".to_context.1.weight", (int64_t)2 * inner * ctx->C), nullptr, 2 * inner);
    free(cn);
  }
  const int Bx = x.B, Hh = x.H, Ww = x.W, HW = x.HW(), nchunk = linattn_chunks(HW);
  const int m = has_ctx ? ctx->HW() : 0;
  T qc = alloc(Bx, Hh, Ww, C3);
  T part = alloc_bytes((size_t)Bx * nchunk * inner * 2 * sizeof(float));
  const Ref qr = at(qc), pr = at(part);
  {
    const Ref xr = at(qkv);
    emit([=](hipStream_t s) { return launch_linattn_dwconv(xr.f(), wdw, qr.f(), pr.f(), Bx, Hh, Ww, inner, s); },
         "linattn dwconv HW" + std::to_string(HW) + " C" + std::to_string(C3), (int64_t)Bx * HW * C3 * 9);
    u->macs += (int64_t)Bx * HW * C3 * 9;
  }
  free(qkv);
  T ctxm = alloc(Bx, H, D, D);
  {
    T ws = alloc_bytes(linattn_ws_floats(Bx, H, HW) * sizeof(float));
    const Ref kr = qr.floats(inner), vr = qr.floats(2 * inner), wr = at(ws), cr = at(ctxm), ck = has_ctx ? at(ckv) : Ref();
    emit([=](hipStream_t s) {
      return launch_linattn_context(kr.f(), vr.f(), C3, pr.f(), HW, ck.f(), ck.floats(inner).f(), 2 * inner, m, nullptr, nullptr,
                                    wr.f(), cr.f(), Bx, H, s);
    }, "linattn context HW" + std::to_string(HW) + " m" + std::to_string(m), (int64_t)Bx * H * (HW + m) * D * D);
    u->macs += (int64_t)Bx * H * (HW + m) * D * D;
    free(ws);
  }
  free(part);
  if (has_ctx) free(ckv);
  T o = alloc(Bx, Hh, Ww, inner);
  {
    const Ref cr = at(ctxm), outr = at(o);
    const float scale = 1.0f / sqrtf((float)D);
    emit([=](hipStream_t s) {
      return launch_linattn_apply(qr.f(), C3, cr.f(), outr.f(), inner, Bx, HW, H, scale, 1, s);
    }, "linattn apply N" + std::to_string(HW), (int64_t)Bx * HW * inner * D);
    u->macs += (int64_t)Bx * HW * inner * D;
  }
  free(qc);
  free(ctxm);
  T proj = linear(o, P(a + ".to_out.0.weight", (int64_t)dim * inner), nullptr, dim);
  free(o);
  T y = feed_forward_tail(x, proj, a + ".to_out.1.g", f, dst);
  free(proj);
  return y;
}

// LinearCrossAttention of feature tokens to the conditioning tokens c; returns attn(x) + x.  The keys / values are the
// learned null pair (shared by every head and image) followed by to_kv(c): their context blocks depend on c alone and are
// computed in the cond region; per step: LayerNorm, to_q's GEMM, the apply (no SiLU), to_out's GEMM and its LayerNorm.
// (q_scale / k_scale of the learned-qk-norm fork load with the module and are not used by the linear form.)
T Builder::linear_cross_attn(const T& x, const std::string& pre, const T& c) {
  const int H = cfg.attn_heads, D = cfg.attn_dim_head, inner = H * D, dim = x.C;
  T xn = layernorm(x, P(pre + ".norm.g", dim), nullptr);
  T q = linear(xn, P(pre + ".to_q.weight", (int64_t)inner * dim), nullptr, inner);
  free(xn);
  const float* nkv = P(pre + ".null_kv", 2 * D);
  const int Bx = x.B, m = c.HW();
  T ctxm;
  {   // a function of c alone (cond region)
    auto ph = cond_scope();
    T kv = linear(c, P(pre + ".to_kv.weight", (int64_t)2 * inner * c.C), nullptr, 2 * inner);
    ctxm = alloc(Bx, H, D, D);
    const Ref kr = at(kv), vr = kr.floats(inner), cr = at(ctxm);
    emit([=](hipStream_t s) {
      return launch_linattn_context(nullptr, nullptr, 0, nullptr, 0, kr.f(), vr.f(), 2 * inner, m, nkv, nkv + D, nullptr, cr.f(),
                                    Bx, H, s);
    }, "linattn xcontext m" + std::to_string(m + 1), (int64_t)Bx * H * (m + 1) * D * D);
    if (phase != Phase::Text) u->macs += (int64_t)Bx * H * (m + 1) * D * D;
    free(kv);
  }
  T o = alloc(Bx, x.H, x.W, inner);
  {
    const Ref qr = at(q), cr = at(ctxm), outr = at(o);
    const int N = x.HW();
    const float scale = 1.0f / sqrtf((float)D);
    emit([=](hipStream_t s) {
      return launch_linattn_apply(qr.f(), inner, cr.f(), outr.f(), inner, Bx, N, H, scale, 0, s);
    }, "linattn xapply N" + std::to_string(N), (int64_t)Bx * N * inner * D);
    u->macs += (int64_t)Bx * N * inner * D;
  }
  free(q);
  free(ctxm);
  T proj = linear(o, P(pre + ".to_out.0.weight", (int64_t)dim * inner), nullptr, dim);
  free(o);
  T y = layernorm(proj, P(pre + ".to_out.1.g", dim), nullptr, &x, ACT_NONE, nullptr, nullptr, true);   // block2's GroupNorm reads it
  free(proj);
  return y;
}

}  // namespace kd
