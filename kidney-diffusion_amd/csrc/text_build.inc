// Builder::build_text(): the step-invariant text-conditioning sub-plan (run once per sample call).
// Mirrors the text branch of Unet.forward in imagen-pytorch 1.18.5 (SURVEY.md Appendix A.1): the
// reference reaches it through sample_cond.py:36-48 / sample.py:51-60 with the seg-cond UNet of
// train.py:30-39 (text_embed_dim 3, one "token" [0.0, 0.5, 0.2], cond_dim 512).
//   tokens  = where(mask & keep, text_to_cond(text_embeds) padded to max_text_len, null_text_embed)
//             (no mask: the padded tokens as they are, where(keep, ., null_text_embed))
//   tokens  = PerceiverResampler(tokens)            (4 mean-pooled + 32 learned latents, depth 2)
//   hiddens = where(keep, to_text_non_attn_cond(mean(tokens)), null_text_hidden)
namespace kd {

void Builder::build_text() {
  const int cd = cfg.cond_dim, H = cfg.attn_heads, D = cfg.attn_dim_head, inner = H * D;
  const int tcd = cfg.dim * 4 * (cfg.lowres_cond ? 2 : 1);
  const int ted = (int)(numel("text_to_cond.weight") / cd);
  const int P = (int)(numel("null_text_embed") / cd);          // max_text_len
  const int n_lat = (int)(numel("attn_pool.latents") / cd);    // 32
  const int n_mp = cfg.text_tokens - n_lat;                    // 4 mean-pooled latents
  if (n_mp <= 0) throw std::runtime_error("text plan: text_tokens must exceed the number of learned latents");
  const int ntok = cfg.text_tokens;
  u->text_embed_dim = ted;
  u->max_text_len = P;
  const kd_unet* io = u;   // the per-call text inputs and output buffers are read through it when an op runs
  const int Bx = B;

  // 1. project + select against the null embedding
  T tok = alloc(B, 1, P, cd);  // rows >= L stay unused
  T x = alloc(B, 1, P, cd);
  {
    const float* w = P_("text_to_cond.weight"), *bias = P_("text_to_cond.bias");
    const float* null_embed = P_("null_text_embed");
    const Ref tr = at(tok), xr = at(x);
    emit([=](hipStream_t s) {
      const int L = io->in_text_len;
      if (L < 1 || L > P || !io->in_text_embeds) {   // (in_text_mask == nullptr: the library's text_mask = None)
        set_error("text conditioning: text_embeds [B,L<=max_text_len,text_embed_dim] are required");
        return 1;
      }
      if (launch_linear_skinny(io->in_text_embeds, ted, w, bias, tr.f(), cd, Bx * L, ted, cd, ACT_NONE, ACT_NONE, s)) return 1;
      return launch_text_select(tr.f(), io->in_text_mask, null_embed, xr.f(), Bx, L, P, cd, io->in_text_drop, s);
    });
  }
  free(tok);

  // 2. PerceiverResampler
  T xp = alloc(B, 1, P, cd);
  {
    const float* pos = P_("attn_pool.pos_emb.weight");
    const Ref xr = at(x), yr = at(xp);
    emit([=](hipStream_t s) { return launch_add_rows_bcast(xr.f(), pos, yr.f(), Bx, P, cd, s); });
  }
  T lat = alloc(B, 1, ntok, cd);
  {
    T mp = alloc(B, 1, 1, cd);
    const Ref xr = at(x), mr = at(mp);
    emit([=](hipStream_t s) { return launch_mean_rows(xr.f(), mr.f(), Bx, P, cd, s); });
    T mpn = layernorm(mp, P_("attn_pool.to_latents_from_mean_pooled_seq.0.g"), nullptr);
    free(mp);
    // Linear(cd -> n_mp*cd) written as the first n_mp rows of every batch's latent block
    skinny(at(mpn), cd, P_("attn_pool.to_latents_from_mean_pooled_seq.1.weight"),
           P_("attn_pool.to_latents_from_mean_pooled_seq.1.bias"), at(lat), ntok * cd, B, cd, n_mp * cd, ACT_NONE,
           ACT_NONE);
    free(mpn);
    const float* latp = P_("attn_pool.latents");
    const Ref lr = at(lat).floats((int64_t)n_mp * cd);
    emit([=](hipStream_t s) {  // learned latents broadcast to every batch element, rows n_mp..ntok
      return launch_copy_rows(latp, 0, cd, lr.f(), (int64_t)ntok * cd, cd, n_lat, cd, Bx, s);
    });
  }
  free(x);
  for (int layer = 0; has("attn_pool.layers." + std::to_string(layer) + ".0.to_q.weight"); ++layer) {
    const std::string a = "attn_pool.layers." + std::to_string(layer) + ".0";
    const std::string f = "attn_pool.layers." + std::to_string(layer) + ".1";
    T xn = layernorm(xp, P_(a + ".norm.weight"), P_(a + ".norm.bias"));
    T ln = layernorm(lat, P_(a + ".norm_latents.weight"), P_(a + ".norm_latents.bias"));
    T q = linear(ln, P_(a + ".to_q.weight"), nullptr, inner);
    T kvx = linear(xn, P_(a + ".to_kv.weight"), nullptr, 2 * inner);
    T kvl = linear(ln, P_(a + ".to_kv.weight"), nullptr, 2 * inner);
    free(xn);
    free(ln);
    if (cfg.attn_qk_norm) {
      qk_norm(q, inner, H, q_scale_of(a));
      qk_norm(kvx, 2 * inner, H, k_scale_of(a));
      qk_norm(kvl, 2 * inner, H, k_scale_of(a));
    }
    T o = alloc(B, 1, ntok, inner);
    {
      const Ref qr = at(q), xr = at(kvx), lr = at(kvl), outr = at(o);
        float scale = attn_scale();
      emit([=](hipStream_t s) {
        KVSeg s0{xr.f(), xr.floats(inner).f(), 2 * inner, P};
        KVSeg s1{lr.f(), lr.floats(inner).f(), 2 * inner, ntok};
        return launch_attention(qr.f(), inner, nullptr, nullptr, s0, s1, outr.f(), inner, Bx, ntok, H, H, D, scale, s);
      });
    }
    free(q);
    free(kvx);
    free(kvl);
    T proj = linear(o, P_(a + ".to_out.0.weight"), nullptr, cd);
    free(o);
    T lat1 = layernorm(proj, P_(a + ".to_out.1.weight"), P_(a + ".to_out.1.bias"), &lat);
    free(proj);
    free(lat);
    const int hidden = (int)(numel(f + ".1.weight") / cd);
    T h0 = layernorm(lat1, P_(f + ".0.g"), nullptr);
    T h1 = linear(h0, P_(f + ".1.weight"), nullptr, hidden, ACT_GELU);
    free(h0);
    T h2 = layernorm(h1, P_(f + ".3.g"), nullptr);
    free(h1);
    lat = linear(h2, P_(f + ".4.weight"), nullptr, cd, ACT_NONE, &lat1);
    free(h2);
    free(lat1);
  }
  free(xp);

  // 3. outputs: pooled tokens and the non-attention text hiddens
  {
    const Ref lr = at(lat);
    emit([=](hipStream_t s) {
      if (!io->out_text_tokens || !io->out_text_hiddens) {
        set_error("text conditioning: output buffers are required");
        return 1;
      }
      return launch_copy_rows(lr.f(), (int64_t)ntok * cd, cd, io->out_text_tokens, (int64_t)ntok * cd, cd, ntok, cd, Bx, s);
    });
    T mean = alloc(B, 1, 1, cd);
    const Ref mr = at(mean);
    emit([=](hipStream_t s) { return launch_mean_rows(lr.f(), mr.f(), Bx, ntok, cd, s); });
    T mn = layernorm(mean, P_("to_text_non_attn_cond.0.weight"), P_("to_text_non_attn_cond.0.bias"));
    free(mean);
    T h = alloc(B, 1, 1, tcd);
    skinny(at(mn), cd, P_("to_text_non_attn_cond.1.weight"), P_("to_text_non_attn_cond.1.bias"), at(h), tcd, B, cd, tcd,
           ACT_NONE, ACT_SILU);
    free(mn);
    T hh = alloc(B, 1, 1, tcd);
    skinny(at(h), tcd, P_("to_text_non_attn_cond.3.weight"), P_("to_text_non_attn_cond.3.bias"), at(hh), tcd, B, tcd,
           tcd, ACT_NONE, ACT_NONE);
    free(h);
    const float* null_hidden = P_("null_text_hidden");
    const Ref hr = at(hh);
    emit([=](hipStream_t s) {
      if (io->in_text_drop)  // cond_drop_prob = 1: every sample takes the learned null hidden
        return launch_copy_rows(null_hidden, 0, tcd, io->out_text_hiddens, tcd, tcd, 1, tcd, Bx, s);
      return launch_copy_rows(hr.f(), tcd, tcd, io->out_text_hiddens, tcd, tcd, 1, tcd, Bx, s);
    });
    free(hh);
  }
  free(lat);
  if (!refs.empty()) throw std::runtime_error("text plan: tensors leaked");
}

}  // namespace kd
