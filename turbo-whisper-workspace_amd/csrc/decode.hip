// Fused Whisper logits processing + greedy selection, one workgroup per batch row, no host sync.
//
// Restates, for num_beams = 1, the per-step work of GenerationMixin._sample
// ($TF/generation/utils.py:2876-2941: f32 logits, processors, argmax = first max, pad after EOS,
// EOS / max_length stopping) with the Whisper processor chain in the order
// WhisperGenerationMixin._retrieve_logit_processors builds it
// ($TF/models/whisper/generation_whisper.py:1774-1812):
//   SuppressTokensAtBeginLogitsProcessor  ($TF/generation/logits_process.py:1816-1866)
//   SuppressTokensLogitsProcessor         (:1869-1906)
//   WhisperTimeStampLogitsProcessor        (:1909-2047)
// The reference loops over rows in Python with .tolist() (a device->host sync per row per step);
// here the processor state (#generated, last two tokens, last timestamp) lives in a device array and
// the masks, the timestamp log-prob rule and the argmax are evaluated in one pass over the vocab.
// Language detection (generation_whisper.py:1610-1673: argmax over the language ids of the first
// decoder step) is mode 1 of the same kernel.
#include "tw_common.h"
#include "../../include/tw_whisper.h"

struct Best {
  float v;
  int i;
};
__device__ inline Best best_of(Best a, Best b) {
  // larger value wins; ties -> smaller index (torch.argmax returns the first maximal index)
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
__device__ inline void lse_merge(float& m, float& s, float m2, float s2) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) { m = m2; s = s2; return; }
  if (m2 > m) { s = s * __expf(m - m2) + s2; m = m2; }
  else s = s + s2 * __expf(m2 - m);
}

// lse_merge(m, s, x, 1) without branches (per logit in the beam partials): d = x - m; x above m rescales s by
// exp(m - x) = exp(-|d|) and adds 1, otherwise s gains exp(d) = exp(-|d|) — the same exp argument and the same
// arithmetic as lse_merge in every case (an -inf x adds exp(-inf) = 0; a first finite x over m = -inf gives
// s * 0 + 1), so the result is bit-identical
__device__ inline void lse_add1(float& m, float& s, float x) {
  const float d = x - m;
  const float e = (x == -INFINITY) ? 0.f : __expf(-fabsf(d));
  s = (d > 0.f) ? s * e + 1.f : s + e;
  m = fmaxf(m, x);
}

// Partial record of one vocab chunk of one row (8 words).
struct SelPart {
  float bt_v; int bt_i;   // best text (or mode-1) candidate
  float bs_v; int bs_i;   // best timestamp candidate
  float m_ts, s_ts;       // logsumexp state over the timestamp logits
  float pad0, pad1;
};

// Row-constant masks of WhisperTimeStampLogitsProcessor.__call__ for this step.
struct RowMask {
  int init_step, mask_ts_all, mask_text_lt_eos, ts_hi_block;
};
__device__ inline RowMask row_mask(const int* st, const TwSelectParams& p) {
  const int n_gen = st[TW_ST_NGEN], last = st[TW_ST_LAST], penult = st[TW_ST_PENULT], last_ts = st[TW_ST_LASTTS];
  const int tsb = p.ts_begin;
  RowMask r{n_gen == 0, 0, 0, tsb};
  if (p.mode == 0 && p.use_timestamps) {
    const bool last_was_ts = n_gen >= 1 && last >= tsb;
    const bool penult_was_ts = n_gen < 2 || penult >= tsb;
    if (last_was_ts) {
      if (penult_was_ts) r.mask_ts_all = 1;
      else r.mask_text_lt_eos = 1;
    }
    if (last_ts >= 0) r.ts_hi_block = (last_was_ts && !penult_was_ts) ? last_ts : last_ts + 1;
  }
  return r;
}

// One vocab chunk [v0, v1) of one row with a 256-thread block (4 waves): the processed (masked) logits' best text and
// best timestamp candidates and the timestamp logsumexp state, reduced to one record in `out` (valid in thread 0).
// TX: also accumulate (per thread, unreduced) the logsumexp state of the unmasked TEXT logits into m_tx / s_tx
// (k_select_full's log_softmax denominator); off, the arithmetic is k_select_partial's exactly.
template <bool TX>
__device__ inline void sel_chunk(const float* __restrict__ row, const uint32_t* __restrict__ suppress_bits,
                                 const TwSelectParams& p, const RowMask& rm, int v0, int v1, SelPart* sp,
                                 SelPart& out, float& m_tx, float& s_tx) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tsb = p.ts_begin;
  Best bt{-INFINITY, 0x7fffffff}, bs{-INFINITY, 0x7fffffff};
  float m_ts = -INFINITY, s_ts = 0.f;
  // 4 loads in flight per thread; indices clamped into the chunk (duplicates are dropped by `ok`)
  for (int base = v0 + tid; base < v1; base += 4 * 256) {
    float xs[4];
    uint32_t sb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = min(base + 256 * u, v1 - 1);
      xs[u] = row[v];
      sb[u] = suppress_bits ? suppress_bits[v >> 5] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = base + 256 * u;
      const bool ok = v < v1;
      float x = xs[u];
      bool masked;
      if (p.mode == 1) {
        masked = (v < p.lo || v >= p.hi);
      } else {
        masked = (sb[u] >> (v & 31)) & 1u;
        if (rm.init_step)
          for (int i = 0; i < p.n_begin_suppress; ++i) masked |= (v == p.begin_suppress[i]);
        if (p.use_timestamps) {
          masked |= (v == p.no_timestamps);
          if (v >= tsb) {
            masked |= rm.mask_ts_all || (v < rm.ts_hi_block);
            if (rm.init_step && p.max_initial_ts >= 0) masked |= (v > tsb + p.max_initial_ts);
          } else {
            masked |= (rm.mask_text_lt_eos && v < p.eos) || rm.init_step;
          }
        }
      }
      if (masked) x = -INFINITY;
      if (!ok) continue;
      if (v < tsb || !p.use_timestamps || p.mode == 1) {
        bt = best_of(bt, Best{x, v});
        if (TX && x != -INFINITY) lse_merge(m_tx, s_tx, x, 1.f);
      } else {
        bs = best_of(bs, Best{x, v});
        if (x != -INFINITY) lse_merge(m_ts, s_ts, x, 1.f);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best ot{__shfl_xor(bt.v, o, 64), __shfl_xor(bt.i, o, 64)};
    Best os{__shfl_xor(bs.v, o, 64), __shfl_xor(bs.i, o, 64)};
    bt = best_of(bt, ot);
    bs = best_of(bs, os);
    float m2 = __shfl_xor(m_ts, o, 64), s2 = __shfl_xor(s_ts, o, 64);
    lse_merge(m_ts, s_ts, m2, s2);
  }
  if (lane == 0) sp[wid] = SelPart{bt.v, bt.i, bs.v, bs.i, m_ts, s_ts, 0.f, 0.f};
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      bt = best_of(bt, Best{sp[w].bt_v, sp[w].bt_i});
      bs = best_of(bs, Best{sp[w].bs_v, sp[w].bs_i});
      lse_merge(m_ts, s_ts, sp[w].m_ts, sp[w].s_ts);
    }
    out = SelPart{bt.v, bt.i, bs.v, bs.i, m_ts, s_ts, 0.f, 0.f};
  }
}

// grid (B, TW_SELECT_CHUNKS): chunk c of row b scans vocab [c*V/NC, (c+1)*V/NC) with float4 loads where aligned.
__global__ TW_DEC_LB(256, 1) void k_select_partial(const float* __restrict__ logits, int ld_logits,
                                                        const uint32_t* __restrict__ suppress_bits, TwSelectParams p,
                                                        const int* __restrict__ state, SelPart* __restrict__ ws) {
  TW_DEC_PRIO();
  __shared__ SelPart sp[4];
  const int b = blockIdx.x, c = blockIdx.y, NC = gridDim.y;
  const RowMask rm = row_mask(state + b * TW_STATE_STRIDE, p);
  const int V = p.V;
  const int v0 = (int)((long)c * V / NC), v1 = (int)((long)(c + 1) * V / NC);
  SelPart out;
  float m_tx = -INFINITY, s_tx = 0.f;
  sel_chunk<false>(logits + (size_t)b * ld_logits, suppress_bits, p, rm, v0, v1, sp, out, m_tx, s_tx);
  if (threadIdx.x == 0) ws[b * NC + c] = out;
}

// Merge of a row's chunk records (in chunk order: ties keep the first index): every lane ends with the row's best
// text / best timestamp candidates and its timestamp logsumexp state.
__device__ inline void sel_merge(const SelPart* __restrict__ ws, int NC, int b, int lane, Best& bt, Best& bs,
                                 float& m_ts, float& s_ts) {
  bt = Best{-INFINITY, 0x7fffffff};
  bs = Best{-INFINITY, 0x7fffffff};
  m_ts = -INFINITY;
  s_ts = 0.f;
  for (int c = lane; c < NC; c += 64) {
    const SelPart r = ws[b * NC + c];
    bt = best_of(bt, Best{r.bt_v, r.bt_i});
    bs = best_of(bs, Best{r.bs_v, r.bs_i});
    lse_merge(m_ts, s_ts, r.m_ts, r.s_ts);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best ot{__shfl_xor(bt.v, o, 64), __shfl_xor(bt.i, o, 64)};
    Best os{__shfl_xor(bs.v, o, 64), __shfl_xor(bs.i, o, 64)};
    bt = best_of(bt, ot);
    bs = best_of(bs, os);
    float m2 = __shfl_xor(m_ts, o, 64), s2 = __shfl_xor(s_ts, o, 64);
    lse_merge(m_ts, s_ts, m2, s2);
  }
}
// The timestamp processor's rule ("if sum of probability over timestamps is above any other token, sample timestamp":
// the text logits are masked when the timestamps' logsumexp beats the best text logit) and the greedy choice.
__device__ inline bool sel_rule_fires(const TwSelectParams& p, Best bt, float m_ts, float s_ts) {
  if (!p.use_timestamps) return false;
  const float lse_ts = (m_ts == -INFINITY) ? -INFINITY : m_ts + __logf(s_ts);
  return lse_ts > bt.v;
}
__device__ inline int sel_greedy(const TwSelectParams& p, Best bt, Best bs, float m_ts, float s_ts) {
  if (!p.use_timestamps) return bt.i;
  return sel_rule_fires(p, bt, m_ts, s_ts) ? bs.i : best_of(bt, bs).i;
}
// _sample's pad-after-EOS / stopping rule and the processor state update for the chosen `sel`; returns the token fed
// to the next step.
__device__ inline int sel_commit(const TwSelectParams& p, int* __restrict__ st, int sel, int* __restrict__ tokens_out,
                                 int ld_tokens, int* __restrict__ next_ids, int b) {
  const int n_gen = st[TW_ST_NGEN], last = st[TW_ST_LAST];
  const int finished = st[TW_ST_FINISHED];
  const int tok = finished ? p.pad : sel;
  if (tokens_out) tokens_out[(size_t)b * ld_tokens + n_gen] = tok;
  if (next_ids) next_ids[b] = tok;
  st[TW_ST_PENULT] = last;
  st[TW_ST_LAST] = tok;
  if (tok >= p.ts_begin && p.use_timestamps) st[TW_ST_LASTTS] = tok;
  st[TW_ST_NGEN] = n_gen + 1;
  if (!finished && (tok == p.eos || n_gen + 1 >= p.max_new)) st[TW_ST_FINISHED] = 1;
  return tok;
}

// One wave per row: merge the row's chunk records, then the selection rule of the timestamp processor, the
// pad-after-EOS / stopping rule of _sample, and the processor state update. Lane 0 returns the token fed to the next
// step (tok) and the row's next position (npos).
__device__ inline void select_final_row(const SelPart* __restrict__ ws, int NC, const TwSelectParams& p,
                                        int* __restrict__ state, int* __restrict__ tokens_out, int ld_tokens,
                                        int* __restrict__ next_ids, int* __restrict__ pos, int b, int lane,
                                        int& tok_out, int& npos) {
  Best bt, bs;
  float m_ts, s_ts;
  sel_merge(ws, NC, b, lane, bt, bs, m_ts, s_ts);
  if (lane != 0) return;
  int* st = state + b * TW_STATE_STRIDE;
  npos = 0;
  if (pos) npos = pos[b] += 1;  // the next decoder step writes its K/V one position later
  if (p.mode == 1) {
    const int sel = bt.i;
    st[TW_ST_LANG] = sel;
    if (next_ids) next_ids[b] = sel;
    tok_out = sel;
    return;
  }
  tok_out = sel_commit(p, st, sel_greedy(p, bt, bs, m_ts, s_ts), tokens_out, ld_tokens, next_ids, b);
}

// grid B, one wave per row
__global__ __launch_bounds__(64) void k_select_final(const SelPart* __restrict__ ws, int NC, TwSelectParams p,
                                                     int* __restrict__ state, int* __restrict__ tokens_out,
                                                     int ld_tokens, int* __restrict__ next_ids,
                                                     int* __restrict__ pos) {
  TW_DEC_PRIO();
  int tok, npos;
  select_final_row(ws, NC, p, state, tokens_out, ld_tokens, next_ids, pos, blockIdx.x, threadIdx.x, tok, npos);
}

// k_select_final fused with the head of the NEXT decoder step (grid B, 256 threads per row): wave 0 selects the
// token, then the block embeds it at the row's next position (embed_tokens + embed_positions, f32 residual
// stream x, as k_embed_decoder) and writes the first layer's self_attn_layer_norm output (as k_resid_ln with no
// partials). Replaces three launches per generated token with one; the results are those of the three.
#define SFE_MAXV 4  // float4 chunks per thread: D <= 4096
template <bool PACKED>
__global__ TW_DEC_LB(256, 1) void k_select_final_embed(const SelPart* __restrict__ ws, int NC, TwSelectParams p,
                                                            int* __restrict__ state, int* __restrict__ tokens_out,
                                                            int ld_tokens, int* __restrict__ next_ids,
                                                            int* __restrict__ pos, const bf16_t* __restrict__ tok_emb,
                                                            const bf16_t* __restrict__ pos_emb, int D, int max_pos,
                                                            float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ bta, float eps,
                                                            bf16_t* __restrict__ out) {
  TW_DEC_PRIO();
  __shared__ float red[8];
  __shared__ int sh[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 64) {
    int tok = 0, npos = 0;
    select_final_row(ws, NC, p, state, tokens_out, ld_tokens, next_ids, pos, b, tid, tok, npos);
    if (tid == 0) {
      sh[0] = tok;
      sh[1] = min(npos, max_pos - 1);  // (past the last step: the embedding is never consumed)
    }
  }
  __syncthreads();
  const bf16_t* te = tok_emb + (size_t)sh[0] * D;
  const bf16_t* pe = pos_emb + (size_t)sh[1] * D;
  float* xr = x + (size_t)b * D;
  const int nc = D >> 2;
  float4 v[SFE_MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < SFE_MAXV; ++i) {
    const int c = min(tid + 256 * i, nc - 1);
    const uint2 t = ((const uint2*)te)[c], q = ((const uint2*)pe)[c];
    float4 a;
    a.x = bf16_to_f32((bf16_t)(t.x & 0xffff)) + bf16_to_f32((bf16_t)(q.x & 0xffff));
    a.y = bf16_to_f32((bf16_t)(t.x >> 16)) + bf16_to_f32((bf16_t)(q.x >> 16));
    a.z = bf16_to_f32((bf16_t)(t.y & 0xffff)) + bf16_to_f32((bf16_t)(q.y & 0xffff));
    a.w = bf16_to_f32((bf16_t)(t.y >> 16)) + bf16_to_f32((bf16_t)(q.y >> 16));
    v[i] = a;
    if (tid + 256 * i < nc) {
      ((float4*)xr)[tid + 256 * i] = a;
      s += (a.x + a.y) + (a.z + a.w);
    }
  }
  tw_row_ln_store<PACKED>(v, s, b, D, eps, g, bta, out, red);
}

extern "C" int tw_logits_select(const float* logits, int B, int ld_logits, const uint32_t* suppress_bits,
                                const TwSelectParams* params, int* state, int* tokens_out, int ld_tokens,
                                int* next_ids, int* pos, float* workspace, void* stream) {
  TW_REQUIRE(logits && params && state && workspace && B > 0, "tw_logits_select: bad args");
  TW_REQUIRE(params->V > 0 && params->V <= ld_logits, "tw_logits_select: V=%d ld=%d", params->V, ld_logits);
  TW_REQUIRE(params->n_begin_suppress >= 0 && params->n_begin_suppress <= 8, "tw_logits_select: begin_suppress");
  static_assert(sizeof(SelPart) * TW_SELECT_CHUNKS == sizeof(float) * TW_SELECT_WS_PER_ROW, "workspace size");
  hipStream_t s = (hipStream_t)stream;
  SelPart* ws = (SelPart*)workspace;
  hipLaunchKernelGGL(k_select_partial, dim3(B, TW_SELECT_CHUNKS), dim3(256), 0, s, logits, ld_logits, suppress_bits,
                     *params, state, ws);
  hipLaunchKernelGGL(k_select_final, dim3(B), dim3(64), 0, s, ws, TW_SELECT_CHUNKS, *params, state, tokens_out,
                     ld_tokens, next_ids, pos);
  return tw_check_launch("tw_logits_select");
}

extern "C" int tw_logits_select_embed(const float* logits, int B, int ld_logits, const uint32_t* suppress_bits,
                                      const TwSelectParams* params, int* state, int* tokens_out, int ld_tokens,
                                      int* next_ids, int* pos, float* workspace, const uint16_t* tok_emb,
                                      const uint16_t* pos_emb, int D, int max_pos, float* x, const float* gamma,
                                      const float* beta, float eps, uint16_t* out, int packed, void* stream) {
  TW_REQUIRE(logits && params && state && workspace && next_ids && pos && B > 0, "tw_logits_select_embed: bad args");
  TW_REQUIRE(params->mode == 0, "tw_logits_select_embed: greedy token selection (mode 0) only");
  TW_REQUIRE(params->V > 0 && params->V <= ld_logits, "tw_logits_select_embed: V=%d ld=%d", params->V, ld_logits);
  TW_REQUIRE(params->n_begin_suppress >= 0 && params->n_begin_suppress <= 8, "tw_logits_select_embed: begin_suppress");
  TW_REQUIRE(tok_emb && pos_emb && x && gamma && beta && out && max_pos > 0, "tw_logits_select_embed: embed/LN args");
  TW_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024 * SFE_MAXV && (!packed || (B <= 64 && D % 32 == 0)),
             "tw_logits_select_embed: D=%d B=%d packed=%d", D, B, packed);
  hipStream_t s = (hipStream_t)stream;
  SelPart* ws = (SelPart*)workspace;
  hipLaunchKernelGGL(k_select_partial, dim3(B, TW_SELECT_CHUNKS), dim3(256), 0, s, logits, ld_logits, suppress_bits,
                     *params, state, ws);
  if (packed)
    hipLaunchKernelGGL(k_select_final_embed<true>, dim3(B), dim3(256), 0, s, ws, TW_SELECT_CHUNKS, *params, state,
                       tokens_out, ld_tokens, next_ids, pos, tok_emb, pos_emb, D, max_pos, x, gamma, beta, eps, out);
  else
    hipLaunchKernelGGL(k_select_final_embed<false>, dim3(B), dim3(256), 0, s, ws, TW_SELECT_CHUNKS, *params, state,
                       tokens_out, ld_tokens, next_ids, pos, tok_emb, pos_emb, D, max_pos, x, gamma, beta, eps, out);
  return tw_check_launch("tw_logits_select_embed");
}

// =================================================================================================
// Temperature fallback (WhisperGenerationMixin.generate_with_fallback, $TF/models/whisper/generation_whisper.py:
// 970-1116): one workgroup per row does the whole selection of a decode step, because the fallback criteria need the
// step's log-probability and sampling needs the row's top-k.
//   * the processors and the chosen greedy token are tw_logits_select's, bit for bit: the row is scanned as the same
//     TW_SELECT_CHUNKS chunks with the same per-thread mapping (sel_chunk) and merged in the same order (sel_merge);
//   * temperature > 0 (do_sample): TemperatureLogitsWarper then TopKLogitsWarper (GenerationConfig's default top_k 50,
//     ties at the k-th value kept: logits_process.py TopKLogitsWarper) and a draw from the softmax of what is left
//     ($TF/generation/utils.py _sample: multinomial) by the Gumbel-max trick — argmax of s/T + G, G = -log(-log U) with
//     U from a counter-based hash of (seed, row key, token index in the pass, vocabulary id): the same distribution as
//     torch.multinomial, not its random stream (sampled tokens are therefore not comparable token for token);
//   * the log-probability of the chosen token under the step's scores as generate() returns them (output_scores: the
//     processed scores, after the warpers when sampling) at temperature 1 — _retrieve_avg_logprobs
//     (generation_whisper.py:1958-1975) — is added to the row's state slot TW_ST_SUMLP (f32 bits) while the row is
//     unfinished (EOS included, pads not).
// =================================================================================================
__device__ inline uint64_t tw_mix64(uint64_t z) {  // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ inline float tw_gumbel(uint64_t seed, uint32_t key, uint32_t step, uint32_t v) {
  const uint64_t h = tw_mix64(seed ^ tw_mix64(((uint64_t)key << 32) ^ ((uint64_t)step << 20) ^ (uint64_t)v));
  const float u = ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);  // (0, 1), 24 bits
  return -logf(-logf(u));
}
// the processed value of vocabulary entry v (the masks of sel_chunk, mode 0)
__device__ inline float sel_processed(const float* __restrict__ row, const uint32_t* __restrict__ suppress_bits,
                                      const TwSelectParams& p, const RowMask& rm, int v) {
  const int tsb = p.ts_begin;
  bool masked = suppress_bits ? (suppress_bits[v >> 5] >> (v & 31)) & 1u : false;
  if (rm.init_step)
    for (int i = 0; i < p.n_begin_suppress; ++i) masked |= (v == p.begin_suppress[i]);
  if (p.use_timestamps) {
    masked |= (v == p.no_timestamps);
    if (v >= tsb) {
      masked |= rm.mask_ts_all || (v < rm.ts_hi_block);
      if (rm.init_step && p.max_initial_ts >= 0) masked |= (v > tsb + p.max_initial_ts);
    } else {
      masked |= (rm.mask_text_lt_eos && v < p.eos) || rm.init_step;
    }
  }
  return masked ? -INFINITY : row[v];
}
__device__ inline float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ inline void block_lse256(float& m, float& s, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[2 * (threadIdx.x >> 6)] = m;
    red[2 * (threadIdx.x >> 6) + 1] = s;
  }
  __syncthreads();
  m = red[0];
  s = red[1];
  for (int w = 1; w < 4; ++w) lse_merge(m, s, red[2 * w], red[2 * w + 1]);
}

// grid B, 256 threads (mode 0)
__global__ __launch_bounds__(256) void k_select_full(const float* __restrict__ logits, int ld_logits,
                                                     const uint32_t* __restrict__ suppress_bits, TwSelectParams p,
                                                     float temperature, int top_k, uint64_t seed,
                                                     const int* __restrict__ row_key, int* __restrict__ state,
                                                     int* __restrict__ tokens_out, int ld_tokens,
                                                     int* __restrict__ next_ids, int* __restrict__ pos,
                                                     float* __restrict__ token_lp, int ld_lp) {
  __shared__ SelPart sp[4];
  __shared__ SelPart parts[TW_SELECT_CHUNKS];
  __shared__ float red[8];
  __shared__ uint32_t hist[256];
  __shared__ int bcast[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  int* st = state + b * TW_STATE_STRIDE;
  const RowMask rm = row_mask(st, p);
  const float* row = logits + (size_t)b * ld_logits;
  const int V = p.V, NC = TW_SELECT_CHUNKS, tsb = p.ts_begin;
  float m_tx = -INFINITY, s_tx = 0.f;
  for (int c = 0; c < NC; ++c) {
    SelPart out;
    sel_chunk<true>(row, suppress_bits, p, rm, (int)((long)c * V / NC), (int)((long)(c + 1) * V / NC), sp, out, m_tx,
                    s_tx);
    if (tid == 0) parts[c] = out;
    __syncthreads();
  }
  block_lse256(m_tx, s_tx, red);  // every thread: the unmasked text logits' logsumexp state
  Best bt, bs;
  float m_ts, s_ts;
  sel_merge(parts, NC, 0, lane, bt, bs, m_ts, s_ts);  // (every wave merges the same records: identical results)
  const bool fire = sel_rule_fires(p, bt, m_ts, s_ts);
  int sel;
  float lse;  // log_softmax denominator of the scores generate() reports for this step
  if (temperature <= 0.f) {
    sel = sel_greedy(p, bt, bs, m_ts, s_ts);
    float m = fire ? -INFINITY : m_tx, sm = fire ? 0.f : s_tx;
    if (p.use_timestamps) lse_merge(m, sm, m_ts, s_ts);
    lse = m + __logf(sm);
  } else {
    // eligible: unmasked after the processors (the rule masks every text logit when it fires)
    const float invT = 1.f / temperature;
    auto elig = [&](int v, float x) { return x != -INFINITY && !(fire && v < tsb); };
    // k-th largest eligible key (f32_order_key of the value: order-preserving), MSB-first radix select
    uint32_t prefix = 0u, mask = 0u;
    int n_el = 0;
    for (int v = tid; v < V; v += 256) n_el += elig(v, sel_processed(row, suppress_bits, p, rm, v)) ? 1 : 0;
    n_el = (int)block_sum256((float)n_el, red);
    const bool restrict_k = top_k > 0 && n_el > top_k;
    if (restrict_k) {
      int k_rem = top_k;
      for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        for (int v = tid; v < V; v += 256) {
          const float x = sel_processed(row, suppress_bits, p, rm, v);
          if (!elig(v, x)) continue;
          const uint32_t key = f32_order_key(x);
          if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          int cum = 0, d = 255;
          for (; d > 0; --d) {
            if (cum + (int)hist[d] >= k_rem) break;
            cum += (int)hist[d];
          }
          bcast[0] = d;
          bcast[1] = k_rem - cum;
        }
        __syncthreads();
        prefix |= (uint32_t)bcast[0] << shift;
        mask |= 255u << shift;
        k_rem = bcast[1];
        __syncthreads();
      }
    }
    // Gumbel-max over the kept set (key >= the k-th largest), and the kept set's logsumexp (scores * T = x)
    const uint32_t rkey = row_key ? (uint32_t)row_key[b] : (uint32_t)b;
    const uint32_t step = (uint32_t)st[TW_ST_NGEN];
    Best g{-INFINITY, 0x7fffffff};
    float m = -INFINITY, sm = 0.f;
    for (int v = tid; v < V; v += 256) {
      const float x = sel_processed(row, suppress_bits, p, rm, v);
      if (!elig(v, x) || (restrict_k && f32_order_key(x) < prefix)) continue;
      lse_merge(m, sm, x, 1.f);
      g = best_of(g, Best{x * invT + tw_gumbel(seed, rkey, step, (uint32_t)v), v});
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) g = best_of(g, Best{__shfl_xor(g.v, o, 64), __shfl_xor(g.i, o, 64)});
    __syncthreads();
    if (lane == 0) {
      red[tid >> 6] = g.v;
      bcast[tid >> 6] = g.i;
    }
    __syncthreads();
    g = Best{red[0], bcast[0]};
    for (int w = 1; w < 4; ++w) g = best_of(g, Best{red[w], bcast[w]});
    sel = g.i;
    block_lse256(m, sm, red);
    lse = m + __logf(sm);
  }
  if (tid != 0) return;
  if (pos) pos[b] += 1;
  const int was_finished = st[TW_ST_FINISHED];
  const int q = st[TW_ST_NGEN];  // the position this step writes
  const int tok = sel_commit(p, st, sel, tokens_out, ld_tokens, next_ids, b);
  float lp = 0.f;  // (a pad after the row finished)
  if (!was_finished) {
    lp = row[tok] - lse;
    st[TW_ST_SUMLP] = __float_as_int(__int_as_float(st[TW_ST_SUMLP]) + lp);
  }
  if (token_lp && q >= 0 && q < ld_lp) token_lp[(size_t)b * ld_lp + q] = lp;
}

// grid B, 256 threads (mode 0), in front of tw_logits_select / _select_embed: the log-probability of the token that
// selection is about to commit, under the step's processed scores — k_select_full's temperature <= 0 branch (the same
// sel_chunk<true> scan, merge, rule and greedy choice on the same inputs, so the same token and the term TW_ST_SUMLP
// sums) without the commit: the row state is only read.
__global__ TW_DEC_LB(256, 1) void k_token_logprob(const float* __restrict__ logits, int ld_logits,
                                                  const uint32_t* __restrict__ suppress_bits, TwSelectParams p,
                                                  const int* __restrict__ state, float* __restrict__ lp_out,
                                                  int ld_lp) {
  TW_DEC_PRIO();
  __shared__ SelPart sp[4];
  __shared__ SelPart parts[TW_SELECT_CHUNKS];
  __shared__ float red[8];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int* st = state + b * TW_STATE_STRIDE;
  const int q = st[TW_ST_NGEN];
  if (q < 0 || q >= ld_lp) return;  // (uniform per block)
  if (st[TW_ST_FINISHED]) {
    if (tid == 0) lp_out[(size_t)b * ld_lp + q] = 0.f;
    return;
  }
  const RowMask rm = row_mask(st, p);
  const float* row = logits + (size_t)b * ld_logits;
  const int V = p.V, NC = TW_SELECT_CHUNKS;
  float m_tx = -INFINITY, s_tx = 0.f;
  for (int c = 0; c < NC; ++c) {
    SelPart out;
    sel_chunk<true>(row, suppress_bits, p, rm, (int)((long)c * V / NC), (int)((long)(c + 1) * V / NC), sp, out, m_tx,
                    s_tx);
    if (tid == 0) parts[c] = out;
    __syncthreads();
  }
  block_lse256(m_tx, s_tx, red);
  Best bt, bs;
  float m_ts, s_ts;
  sel_merge(parts, NC, 0, lane, bt, bs, m_ts, s_ts);
  if (tid != 0) return;
  const bool fire = sel_rule_fires(p, bt, m_ts, s_ts);
  const int sel = sel_greedy(p, bt, bs, m_ts, s_ts);
  float m = fire ? -INFINITY : m_tx, sm = fire ? 0.f : s_tx;
  if (p.use_timestamps) lse_merge(m, sm, m_ts, s_ts);
  lp_out[(size_t)b * ld_lp + q] = row[sel] - (m + __logf(sm));
}

// grid B, 256 threads: softmax(raw logits)[token] into the state slot TW_ST_NOSPEECH (f32 bits)
__global__ __launch_bounds__(256) void k_token_prob(const float* __restrict__ logits, int ld_logits, int V, int token,
                                                    int* __restrict__ state) {
  __shared__ float red[8];
  const float* row = logits + (size_t)blockIdx.x * ld_logits;
  float m = -INFINITY, s = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) lse_merge(m, s, row[v], 1.f);
  block_lse256(m, s, red);
  if (threadIdx.x == 0)
    state[blockIdx.x * TW_STATE_STRIDE + TW_ST_NOSPEECH] = __float_as_int(__expf(row[token] - (m + __logf(s))));
}

extern "C" int tw_logits_sample_lp(const float* logits, int B, int ld_logits, const uint32_t* suppress_bits,
                                   const TwSelectParams* params, float temperature, int top_k, uint64_t seed,
                                   const int* row_key, int* state, int* tokens_out, int ld_tokens, int* next_ids,
                                   int* pos, float* token_lp, int ld_lp, void* stream) {
  TW_REQUIRE(logits && params && state && B > 0, "tw_logits_sample: bad args");
  TW_REQUIRE(params->mode == 0, "tw_logits_sample: generation steps (mode 0) only");
  TW_REQUIRE(params->V > 0 && params->V <= ld_logits, "tw_logits_sample: V=%d ld=%d", params->V, ld_logits);
  TW_REQUIRE(params->n_begin_suppress >= 0 && params->n_begin_suppress <= 8, "tw_logits_sample: begin_suppress");
  TW_REQUIRE(temperature >= 0.f && temperature == temperature, "tw_logits_sample: temperature %f", temperature);
  TW_REQUIRE(!token_lp || ld_lp > 0, "tw_logits_sample_lp: ld_lp=%d", ld_lp);
  hipLaunchKernelGGL(k_select_full, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ld_logits, suppress_bits,
                     *params, temperature, top_k, seed, row_key, state, tokens_out, ld_tokens, next_ids, pos,
                     token_lp, ld_lp);
  return tw_check_launch("tw_logits_sample");
}

extern "C" int tw_logits_sample(const float* logits, int B, int ld_logits, const uint32_t* suppress_bits,
                                const TwSelectParams* params, float temperature, int top_k, uint64_t seed,
                                const int* row_key, int* state, int* tokens_out, int ld_tokens, int* next_ids,
                                int* pos, void* stream) {
  return tw_logits_sample_lp(logits, B, ld_logits, suppress_bits, params, temperature, top_k, seed, row_key, state,
                             tokens_out, ld_tokens, next_ids, pos, nullptr, 0, stream);
}

extern "C" int tw_token_logprob(const float* logits, int B, int ld_logits, const uint32_t* suppress_bits,
                                const TwSelectParams* params, const int* state, float* lp_out, int ld_lp,
                                void* stream) {
  TW_REQUIRE(logits && params && state && lp_out && B > 0 && ld_lp > 0, "tw_token_logprob: bad args");
  TW_REQUIRE(params->mode == 0, "tw_token_logprob: generation steps (mode 0) only");
  TW_REQUIRE(params->V > 0 && params->V <= ld_logits, "tw_token_logprob: V=%d ld=%d", params->V, ld_logits);
  TW_REQUIRE(params->n_begin_suppress >= 0 && params->n_begin_suppress <= 8, "tw_token_logprob: begin_suppress");
  hipLaunchKernelGGL(k_token_logprob, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ld_logits, suppress_bits,
                     *params, state, lp_out, ld_lp);
  return tw_check_launch("tw_token_logprob");
}

extern "C" int tw_token_prob(const float* logits, int B, int ld_logits, int V, int token, int* state, void* stream) {
  TW_REQUIRE(logits && state && B > 0 && V > 0 && V <= ld_logits && token >= 0 && token < V,
             "tw_token_prob: B=%d V=%d token=%d", B, V, token);
  hipLaunchKernelGGL(k_token_prob, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ld_logits, V, token, state);
  return tw_check_launch("tw_token_prob");
}

// =================================================================================================
// Teacher-forced selection (forced alignment): the step's token is given, not chosen. grid B, 256 threads per row,
// in tw_logits_select's place in a decode step. n = state[b][TW_ST_NGEN]; while n < force_len[b] the row commits
// force[b][n] with its log-probability under the RAW logits (f32 log_softmax over [0, V): no processors, nothing is
// being chosen), afterwards it is finished and feeds pad. pos advances either way, so a captured step replays
// unchanged for as many steps as the longest row needs, with no finished check on the host.
// Every index the kernel forms is bounded by its own ld (a forced id outside [0, V) reads no logit: its lp is NaN;
// the TW_DEBUG build reports it instead).
// =================================================================================================
__global__ TW_DEC_LB(256, 1) void k_logits_force(const float* __restrict__ logits, int ld_logits, int V,
                                                 const int* __restrict__ force, int ld_force,
                                                 const int* __restrict__ force_len, int pad, int* __restrict__ state,
                                                 int* __restrict__ tokens_out, int ld_tokens,
                                                 int* __restrict__ next_ids, int* __restrict__ pos,
                                                 float* __restrict__ lp_out, int ld_lp) {
  TW_DEC_PRIO();
  __shared__ float red[8];
  const int b = blockIdx.x, tid = threadIdx.x;
  int* st = state + b * TW_STATE_STRIDE;
  const int n = st[TW_ST_NGEN];  // (thread 0 rewrites it behind block_lse256's barriers)
  const int flen = min(force_len[b], ld_force);
  if (n < 0 || n >= flen) {  // (uniform per block) past the row's end
    if (tid == 0) {
      if (pos) pos[b] += 1;
      st[TW_ST_FINISHED] = 1;
      next_ids[b] = pad;
      if (n >= 0 && n < ld_tokens) tokens_out[(size_t)b * ld_tokens + n] = pad;
      if (n >= 0 && n < ld_lp) lp_out[(size_t)b * ld_lp + n] = 0.f;
    }
    return;
  }
  const int tok = force[(size_t)b * ld_force + n];
  const float* row = logits + (size_t)b * ld_logits;
  float m = -INFINITY, s = 0.f;
  for (int v = tid; v < V; v += 256) lse_merge(m, s, row[v], 1.f);
  block_lse256(m, s, red);
  if (tid != 0) return;
  if (pos) pos[b] += 1;
  const float lp = (tok >= 0 && tok < V) ? row[tok] - (m + logf(s)) : __int_as_float(0x7fc00000);
  if (n < ld_lp) lp_out[(size_t)b * ld_lp + n] = lp;
  if (n < ld_tokens) tokens_out[(size_t)b * ld_tokens + n] = tok;
  next_ids[b] = tok;
  st[TW_ST_PENULT] = st[TW_ST_LAST];
  st[TW_ST_LAST] = tok;
  st[TW_ST_NGEN] = n + 1;
}

#if TW_DEBUG
// Debug builds: outside a graph capture, every forced id the launch is about to commit is checked against [0, V)
// first (the check synchronises the stream) and the call fails with TW_ERR_ARG instead of yielding a NaN.
__global__ __launch_bounds__(64) void k_force_check(const int* __restrict__ force, int ld_force,
                                                    const int* __restrict__ force_len, const int* __restrict__ state,
                                                    int V, int B, int* __restrict__ bad) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int n = state[b * TW_STATE_STRIDE + TW_ST_NGEN];
  int r = 0;
  if (n >= 0 && n < min(force_len[b], ld_force)) {
    const int tok = force[(size_t)b * ld_force + n];
    r = (tok < 0 || tok >= V) ? 1 : 0;
  }
  bad[b] = r;
}
static int tw_debug_force_guard(const int* force, int ld_force, const int* force_len, const int* state, int V, int B,
                                hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return TW_OK;
  static int* d_bad = nullptr;
  static int cap = 0;
  if (cap < B) {
    if (d_bad) (void)hipFree(d_bad);
    cap = 0;
    if (hipMalloc(&d_bad, sizeof(int) * B) != hipSuccess) {
      d_bad = nullptr;
      tw_set_error("tw_logits_force (debug): hipMalloc failed");
      return TW_ERR_LAUNCH;
    }
    cap = B;
  }
  hipLaunchKernelGGL(k_force_check, dim3(tw_cdiv(B, 64)), dim3(64), 0, st, force, ld_force, force_len, state, V, B,
                     d_bad);
  int* h = (int*)alloca(sizeof(int) * B);
  if (hipMemcpyAsync(h, d_bad, sizeof(int) * B, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    tw_set_error("tw_logits_force (debug): the forced-id check failed to run");
    return TW_ERR_LAUNCH;
  }
  for (int b = 0; b < B; ++b)
    if (h[b]) {
      tw_set_error("tw_logits_force: precondition violated: row %d's next forced id is outside [0, %d)", b, V);
      return TW_ERR_ARG;
    }
  return TW_OK;
}
#endif

extern "C" int tw_logits_force(const float* logits, int B, int ld_logits, int V, const int* force, int ld_force,
                               const int* force_len, int pad, int* state, int* tokens_out, int ld_tokens,
                               int* next_ids, int* pos, float* lp_out, int ld_lp, void* stream) {
  TW_REQUIRE(logits && force && force_len && state && tokens_out && next_ids && lp_out,
             "tw_logits_force: null pointer");
  TW_REQUIRE(B > 0 && ld_force > 0 && ld_tokens > 0 && ld_lp > 0, "tw_logits_force: B=%d ld_force=%d ld_tokens=%d "
             "ld_lp=%d", B, ld_force, ld_tokens, ld_lp);
  TW_REQUIRE(V > 0 && V <= ld_logits, "tw_logits_force: V=%d ld=%d", V, ld_logits);
#if TW_DEBUG
  if (int rc = tw_debug_force_guard(force, ld_force, force_len, state, V, B, (hipStream_t)stream)) return rc;
#endif
  hipLaunchKernelGGL(k_logits_force, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ld_logits, V, force, ld_force,
                     force_len, pad, state, tokens_out, ld_tokens, next_ids, pos, lp_out, ld_lp);
  return tw_check_launch("tw_logits_force");
}

// =================================================================================================
// History processors in front of the Whisper chain: RepetitionPenaltyLogitsProcessor
// ($TF/generation/logits_process.py: gather, where(score < 0, score * p, score / p), scatter) then
// NoRepeatNGramLogitsProcessor (_calc_banned_ngram_tokens: every token that followed an earlier occurrence of the
// history's last n-1 tokens is set to -inf), in that order, as _get_logits_processor puts them before the
// model-specific processors. One workgroup (1024 threads) per row, a thread per history position.
//   history of row r = prefix[r][0 .. prefix_len[r]) ++ tokens[r][0 .. state[r][TW_ST_NGEN])
//   (a prefix entry TW_HIST_LANG stands for the row's detected language, state[r][TW_ST_LANG]);
//   to_logprobs: the row is first rewritten to log_softmax over [0, V) (beam search runs its processors on
//   log-probabilities, $TF/generation/utils.py:3270-3275).
// The penalty touches each distinct id once, from the value before any penalty (only the first occurrence's thread
// reads and writes its id); a barrier separates it from the bans, so -inf wins. IEEE f32 multiply / divide (no
// fast-math in this build): the values equal torch's f32 bit for bit. Finished rows and columns [V, ld) are left alone.
//
// With a TwSeqBias table (BIAS; tw_logits_history_bias) two more stages run on the same staged history:
// SequenceBiasLogitsProcessor in front of the penalty (entries [0, n_pre)) and NoBadWordsLogitsProcessor — the same
// processor with -inf biases — behind the bans (entries [n_pre, n_pre + n_post)); generate()'s order is sequence bias,
// penalty, n-gram, bad words. A thread per entry first decides whether the entry fires: a 1-id entry always does, an
// entry of n ids when n <= L and its first n - 1 ids equal the history's last n - 1 (transformers skips
// len > input_ids.shape[1], so n == L + 1 never fires although its prefix would fit). s_last[e] is the fired entry's
// last id, else -1. Then, per stage, the first fired entry that ends in an id owns it: that thread alone adds the
// fired entries' biases that end in the id in table order, from 0.0f, and does one row[id] += total. This is
// transformers' f32 sum (bias = zeros; += length_1_bias — the host puts 1-id entries first —; += each matching entry in
// dict order; scores + bias) without atomics and whatever the thread schedule; entries that do not fire add 0.0 there,
// which changes no f32 sum that started from +0.0. Barriers separate the stages: they may touch the same id.
// =================================================================================================
#define TW_HIST_THREADS 1024
#define TW_HIST_INFLIGHT 8  // logits of a thread's share loaded per trip (one load per trip serialised ~100 round trips)

// one stage of the staged table, entries [e0, e1): see above
__device__ inline void seqbias_stage(float* __restrict__ row, const int* s_last, const float* s_bias, int e0, int e1,
                                     int tid) {
  for (int e = e0 + tid; e < e1; e += TW_HIST_THREADS) {
    const int id = s_last[e];
    if (id < 0) continue;
    // (both loops branch-free and unrolled, so that their LDS reads overlap: one read per trip serialised ~100 LDS
    // round trips per stage; + 0.0f changes no total, which is never -0.0)
    bool owner = true;
#pragma unroll 8
    for (int j = e0; j < e; ++j) owner &= (s_last[j] != id);
    if (!owner) continue;
    float total = 0.f;
#pragma unroll 8
    for (int j = e; j < e1; ++j) total += (s_last[j] == id) ? s_bias[j] : 0.f;
    row[id] += total;
  }
}

template <bool BIAS>
__global__ __launch_bounds__(TW_HIST_THREADS) void k_logits_history(float* __restrict__ logits, int ld_logits, int V,
                                                                    const int* __restrict__ prefix, int ld_prefix,
                                                                    const int* __restrict__ prefix_len,
                                                                    const int* __restrict__ tokens, int ld_tokens,
                                                                    const int* __restrict__ state, float penalty,
                                                                    int ngram, int to_logprobs, TwSeqBias sb) {
  TW_DEC_PRIO();
  __shared__ int h[TW_HIST_MAX];
  __shared__ float red[2 * (TW_HIST_THREADS / 64)];
  __shared__ int s_last[BIAS ? TW_SEQBIAS_MAX_ENTRIES : 1];
  __shared__ float s_bias[BIAS ? TW_SEQBIAS_MAX_ENTRIES : 1];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int* st = state + r * TW_STATE_STRIDE;
  if (st[TW_ST_FINISHED]) return;  // (uniform per block)
  float* row = logits + (size_t)r * ld_logits;
  const int pl = prefix ? min(max(prefix_len[r], 0), ld_prefix) : 0;
  const int ng = min(max(st[TW_ST_NGEN], 0), ld_tokens);
  const int L = min(pl + ng, TW_HIST_MAX);
  for (int i = tid; i < L; i += TW_HIST_THREADS) {
    int id = i < pl ? prefix[(size_t)r * ld_prefix + i] : tokens[(size_t)r * ld_tokens + (i - pl)];
    if (id == TW_HIST_LANG) id = st[TW_ST_LANG];
    h[i] = id;
  }
  if (to_logprobs) {
    float m = -INFINITY, s = 0.f;
    for (int base = tid; base < V; base += TW_HIST_INFLIGHT * TW_HIST_THREADS) {
      float xs[TW_HIST_INFLIGHT];
#pragma unroll
      for (int u = 0; u < TW_HIST_INFLIGHT; ++u) {
        const int v = base + u * TW_HIST_THREADS;
        xs[u] = v < V ? row[v] : -INFINITY;
      }
#pragma unroll
      for (int u = 0; u < TW_HIST_INFLIGHT; ++u) {  // online logsumexp, branch-free (as lse_add1, with expf)
        const float x = xs[u], d = x - m;
        const float e = (x == -INFINITY) ? 0.f : expf(-fabsf(d));
        s = (d > 0.f) ? s * e + 1.f : s + e;
        m = fmaxf(m, x);
      }
    }
    auto merge = [](float& m, float& s, float m2, float s2) {
      if (m2 == -INFINITY) return;
      if (m == -INFINITY) { m = m2; s = s2; return; }
      if (m2 > m) { s = s * expf(m - m2) + s2; m = m2; }
      else s = s + s2 * expf(m2 - m);
    };
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if ((tid & 63) == 0) {
      red[2 * (tid >> 6)] = m;
      red[2 * (tid >> 6) + 1] = s;
    }
    __syncthreads();
    m = red[0];
    s = red[1];
    for (int w = 1; w < TW_HIST_THREADS / 64; ++w) merge(m, s, red[2 * w], red[2 * w + 1]);
    const float lse = m + logf(s);
    for (int base = tid; base < V; base += TW_HIST_INFLIGHT * TW_HIST_THREADS) {
      float xs[TW_HIST_INFLIGHT];
#pragma unroll
      for (int u = 0; u < TW_HIST_INFLIGHT; ++u) {
        const int v = base + u * TW_HIST_THREADS;
        xs[u] = v < V ? row[v] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < TW_HIST_INFLIGHT; ++u) {
        const int v = base + u * TW_HIST_THREADS;
        if (v < V) row[v] = xs[u] - lse;
      }
    }
  }
  __syncthreads();  // h is staged; the row's log-probabilities are written
  if (BIAS) {
    const int ne = sb.n_pre + sb.n_post;
    for (int e = tid; e < ne; e += TW_HIST_THREADS) {
      // the entry's row, length and bias are loaded together (a loop bounded by the loaded length would serialise
      // one round trip per id)
      const int* ids = sb.ids + (size_t)e * sb.ld_ids;
      int idv[TW_SEQBIAS_MAX_IDS];
#pragma unroll
      for (int k = 0; k < TW_SEQBIAS_MAX_IDS; ++k) idv[k] = k < sb.ld_ids ? ids[k] : -1;
      const int n = sb.len[e];
      const float b = sb.bias[e];
      bool fires = n >= 1 && n <= sb.ld_ids && (n == 1 || n <= L);
      int last = -1;
#pragma unroll
      for (int k = 0; k < TW_SEQBIAS_MAX_IDS; ++k) {
        if (k < n - 1) fires = fires && (h[L - (n - 1) + k] == idv[k]);  // (fires: n <= L, the index is in [0, L))
        if (k == n - 1) last = idv[k];
      }
      s_last[e] = (fires && last >= 0 && last < V) ? last : -1;
      s_bias[e] = b;
    }
    __syncthreads();
    seqbias_stage(row, s_last, s_bias, 0, sb.n_pre, tid);
    __syncthreads();  // the penalty reads the biased values
  }
  if (penalty != 1.0f) {
    for (int i = tid; i < L; i += TW_HIST_THREADS) {
      const int id = h[i];
      if (id < 0 || id >= V) continue;
      bool first = true;
      for (int j = 0; j < i; ++j) first &= (h[j] != id);
      if (!first) continue;
      const float x = row[id];
      row[id] = x < 0.f ? x * penalty : x / penalty;
    }
  }
  __syncthreads();  // the bans come after every penalised value
  if (ngram > 0 && L >= ngram) {
    const int tail0 = L - ngram + 1;  // the history's last n-1 tokens start here
    for (int i = tid; i <= L - ngram; i += TW_HIST_THREADS) {
      bool match = true;
      for (int k = 0; k < ngram - 1; ++k) match &= (h[i + k] == h[tail0 + k]);
      const int id = h[i + ngram - 1];
      if (match && id >= 0 && id < V) row[id] = -INFINITY;
    }
  }
  if (BIAS) {
    __syncthreads();  // bad words come after the bans
    seqbias_stage(row, s_last, s_bias, sb.n_pre, sb.n_pre + sb.n_post, tid);
  }
}

extern "C" int tw_logits_history_bias(float* logits, int R, int ld_logits, int V, const int* prefix, int ld_prefix,
                                      const int* prefix_len, const int* tokens, int ld_tokens, const int* state,
                                      float repetition_penalty, int no_repeat_ngram, int to_logprobs,
                                      const TwSeqBias* table, void* stream) {
  TW_REQUIRE(logits && tokens && state && R > 0, "tw_logits_history: bad args");
  TW_REQUIRE(V > 0 && V <= ld_logits, "tw_logits_history: V=%d ld=%d", V, ld_logits);
  TW_REQUIRE((prefix == nullptr) == (prefix_len == nullptr) && ld_prefix >= 0 && ld_tokens >= 0,
             "tw_logits_history: prefix / prefix_len go together (ld_prefix=%d ld_tokens=%d)", ld_prefix, ld_tokens);
  TW_REQUIRE(repetition_penalty > 0.f && repetition_penalty == repetition_penalty && no_repeat_ngram >= 0,
             "tw_logits_history: repetition_penalty=%f no_repeat_ngram=%d", repetition_penalty, no_repeat_ngram);
  TwSeqBias sb = {};
  if (table) {
    TW_REQUIRE(table->n_pre >= 0 && table->n_post >= 0 && table->n_pre <= TW_SEQBIAS_MAX_ENTRIES &&
                   table->n_post <= TW_SEQBIAS_MAX_ENTRIES && table->n_pre + table->n_post <= TW_SEQBIAS_MAX_ENTRIES,
               "tw_logits_history_bias: n_pre=%d + n_post=%d entries exceed TW_SEQBIAS_MAX_ENTRIES=%d", table->n_pre,
               table->n_post, TW_SEQBIAS_MAX_ENTRIES);
    if (table->n_pre + table->n_post > 0) {
      TW_REQUIRE(table->ld_ids >= 1 && table->ld_ids <= TW_SEQBIAS_MAX_IDS,
                 "tw_logits_history_bias: ld_ids=%d (1 .. TW_SEQBIAS_MAX_IDS=%d ids per entry)", table->ld_ids,
                 TW_SEQBIAS_MAX_IDS);
      TW_REQUIRE(table->ids && table->len && table->bias, "tw_logits_history_bias: table arrays missing");
      sb = *table;
    }
  }
  if (sb.n_pre + sb.n_post > 0)
    hipLaunchKernelGGL(k_logits_history<true>, dim3(R), dim3(TW_HIST_THREADS), 0, (hipStream_t)stream, logits,
                       ld_logits, V, prefix, ld_prefix, prefix_len, tokens, ld_tokens, state, repetition_penalty,
                       no_repeat_ngram, to_logprobs, sb);
  else
    hipLaunchKernelGGL(k_logits_history<false>, dim3(R), dim3(TW_HIST_THREADS), 0, (hipStream_t)stream, logits,
                       ld_logits, V, prefix, ld_prefix, prefix_len, tokens, ld_tokens, state, repetition_penalty,
                       no_repeat_ngram, to_logprobs, sb);
  return tw_check_launch("tw_logits_history");
}

extern "C" int tw_logits_history(float* logits, int R, int ld_logits, int V, const int* prefix, int ld_prefix,
                                 const int* prefix_len, const int* tokens, int ld_tokens, const int* state,
                                 float repetition_penalty, int no_repeat_ngram, int to_logprobs, void* stream) {
  return tw_logits_history_bias(logits, R, ld_logits, V, prefix, ld_prefix, prefix_len, tokens, ld_tokens, state,
                                repetition_penalty, no_repeat_ngram, to_logprobs, nullptr, stream);
}

// =================================================================================================
// Beam search (num_beams > 1): GenerationMixin._beam_search ($TF/generation/utils.py:3208-3512) with the same Whisper
// processor chain, early_stopping=False, one EOS id. Rows are window-major: row = w * nb + j.
//   k_beam_partial  grid (R, NC): per vocab chunk of a row, the log-sum-exp of the raw logits (log_softmax), the
//                   timestamp-rule statistics of k_select_partial, and the top-K masked text and timestamp
//                   candidates (K = 2 nb continuations per window, :3277-3282)
//   k_beam_step     grid W: per window, the row candidates (the timestamp rule removes the text ones when it fires),
//                   the window's top-K by accumulated log-prob (:3316-3349), running beams for the next step
//                   (:3131-3151), finished beams (:3153-3206), the early-stop heuristic (:3008-3073); then it
//                   reorders the running token histories, the processor state, ids/pos, and writes the row each
//                   new running beam continues (for the self-attention K/V reorder, tw_kv_reorder)
// =================================================================================================
struct Cand {
  float v;
  int i;
};
// (bitwise, not short-circuit: the || / && form compiled to exec-mask branches around every compare, which set the
// beam kernels' time)
__device__ inline bool cand_better(float v, int i, const Cand& c) { return (v > c.v) | ((v == c.v) & (i < c.i)); }

// Sorted insert as a compare-swap chain: every index is static, so the list stays in VGPRs (the shifting form with
// an early return was lowered to scratch: 80-272 B/lane, k_beam_partial 139 us per step at 60 rows).
template <int K>
__device__ inline void cand_insert(Cand (&L)[K], float v, int i) {
  if (!cand_better(v, i, L[K - 1])) return;
  Cand c{v, i};
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const bool better = cand_better(c.v, c.i, L[j]);
    const Cand o = L[j];
    L[j] = better ? c : o;
    c = better ? o : c;
  }
}

// The wave's best (v, i, l) under the strict order "v higher, then i lower, then lane l lower", in every lane. DPP
// within each 16-lane row (quad xor 1, xor 2, half-row mirror, row mirror: every lane of a row meets every other),
// then the four rows' winners by readlane: ~4x shorter than a 6-level ds_bpermute butterfly (__shfl_xor), whose
// latency chain set most of the beam kernels' time (K dependent rounds per list; k_beam_step 22 of 34 us). The order
// is total, so the winner (and every later round) is the one the butterfly found.
__device__ inline void wave_best(float& bv, int& bi, int& bl) {
  auto step = [&](auto ctrl_tag) {
    constexpr int ctrl = decltype(ctrl_tag)::value;
    const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(bv), ctrl, 0xF, 0xF, false));
    const int oi = __builtin_amdgcn_update_dpp(0, bi, ctrl, 0xF, 0xF, false);
    const int ol = __builtin_amdgcn_update_dpp(0, bl, ctrl, 0xF, 0xF, false);
    const bool b = (ov > bv) | ((ov == bv) & ((oi < bi) | ((oi == bi) & (ol < bl))));
    bv = b ? ov : bv;
    bi = b ? oi : bi;
    bl = b ? ol : bl;
  };
  step(std::integral_constant<int, 0xB1>{});   // quad_perm [1, 0, 3, 2]
  step(std::integral_constant<int, 0x4E>{});   // quad_perm [2, 3, 0, 1]
  step(std::integral_constant<int, 0x141>{});  // row_half_mirror
  step(std::integral_constant<int, 0x140>{});  // row_mirror
  float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bv), 0));
  int i = __builtin_amdgcn_readlane(bi, 0), l = __builtin_amdgcn_readlane(bl, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) {
    const float ov = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bv), r));
    const int oi = __builtin_amdgcn_readlane(bi, r), ol = __builtin_amdgcn_readlane(bl, r);
    const bool b = (ov > v) | ((ov == v) & ((oi < i) | ((oi == i) & (ol < l))));
    v = b ? ov : v;
    i = b ? oi : i;
    l = b ? ol : l;
  }
  bv = v;
  bi = i;
  bl = l;
}

// K rounds of wave argmax over the lanes' sorted lists: out (LDS, K entries) = the wave's top-K, descending.
template <int K>
__device__ inline void wave_topk(Cand (&L)[K], Cand* out, int lane) {
  for (int r = 0; r < K; ++r) {
    float bv = L[0].v;
    int bi = L[0].i, bl = lane;
    wave_best(bv, bi, bl);
    if (lane == 0) out[r] = Cand{bv, bi};
    const bool pop = lane == bl;  // pop the head (selects, not a branch around register moves)
#pragma unroll
    for (int j = 0; j < K - 1; ++j) L[j] = pop ? L[j + 1] : L[j];
    L[K - 1] = pop ? Cand{-INFINITY, 0x7fffffff} : L[K - 1];
  }
}

template <int K>
struct BeamPart {
  Cand t[K];  // top-K masked text candidates (logit value)
  Cand s[K];  // top-K masked timestamp candidates
  float m_all, s_all, m_ts, s_ts;
  float m_tx, s_tx;  // (renorm) log-sum-exp of the allowed text tokens
};

// -DTW_BEAM_PROBE (measurement builds only, never the product library): per-phase timestamps of block 0 of the two
// beam kernels (100 MHz s_memrealtime, thread 0), read back with tw_beam_probe_read
#ifdef TW_BEAM_PROBE
__device__ unsigned long long tw_beam_probe_ts[2][16];
#define BPROBE(k, slot) \
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) tw_beam_probe_ts[k][slot] = __builtin_amdgcn_s_memrealtime()
extern "C" int tw_beam_probe_read(unsigned long long* host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(tw_beam_probe_ts), sizeof(tw_beam_probe_ts)) == hipSuccess ? 0 : 1;
}
#else
#define BPROBE(k, slot)
#endif

template <int K>
__global__ __launch_bounds__(256) void k_beam_partial(const float* __restrict__ logits, int ld_logits,
                                                      const uint32_t* __restrict__ suppress_bits, TwSelectParams p,
                                                      const int* __restrict__ state, BeamPart<K>* __restrict__ ws,
                                                      int renorm) {
  TW_DEC_PRIO();
  BPROBE(0, 0);
  __shared__ Cand wl[2][4][K];
  __shared__ float wst[4][6];
  const int b = blockIdx.x, c = blockIdx.y, NC = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const RowMask rm = row_mask(state + b * TW_STATE_STRIDE, p);
  const float* row = logits + (size_t)b * ld_logits;
  const int V = p.V, tsb = p.ts_begin;
  // with timestamps the last chunk is exactly the timestamp tokens and the others split the text tokens, so no block
  // holds both kinds: each reduces one candidate list (the block holding both set the launch's duration)
  const bool split_ts = p.use_timestamps && tsb > 0 && tsb < V && NC > 1;
  const int v0 = split_ts ? (c == NC - 1 ? tsb : (int)((long)c * tsb / (NC - 1))) : (int)((long)c * V / NC);
  const int v1 = split_ts ? (c == NC - 1 ? V : (int)((long)(c + 1) * tsb / (NC - 1))) : (int)((long)(c + 1) * V / NC);
  Cand T[K], S[K];
#pragma unroll
  for (int j = 0; j < K; ++j) T[j] = S[j] = Cand{-INFINITY, 0x7fffffff};
  float m_all = -INFINITY, s_all = 0.f, m_ts = -INFINITY, s_ts = 0.f, m_tx = -INFINITY, s_tx = 0.f;
  auto visit = [&](int v, float x, uint32_t sbw) {
    lse_add1(m_all, s_all, x);
    bool masked = (sbw >> (v & 31)) & 1u;
    if (rm.init_step)
      for (int i = 0; i < p.n_begin_suppress; ++i) masked |= (v == p.begin_suppress[i]);
    if (p.use_timestamps) {
      masked |= (v == p.no_timestamps);
      if (v >= tsb) {
        masked |= rm.mask_ts_all || (v < rm.ts_hi_block);
        if (rm.init_step && p.max_initial_ts >= 0) masked |= (v > tsb + p.max_initial_ts);
      } else {
        masked |= (rm.mask_text_lt_eos && v < p.eos) || rm.init_step;
      }
    }
    if (masked) return;
    if (v < tsb || !p.use_timestamps) {
      cand_insert<K>(T, x, v);
      if (renorm) lse_add1(m_tx, s_tx, x);
    } else {
      cand_insert<K>(S, x, v);
      lse_add1(m_ts, s_ts, x);
    }
  };
  // every logit (and suppress word) of this thread's share in flight at once: one load per loop trip serialised ~13
  // memory round trips (57 us per launch at 60 rows); a share past BP_MAXE per thread (V > 65536) takes the tail loop
  constexpr int BP_MAXE = 16;
  float xs[BP_MAXE];
  uint32_t sb[BP_MAXE];
#pragma unroll
  for (int u = 0; u < BP_MAXE; ++u) {
    const int v = min(v0 + tid + 256 * u, v1 - 1);
    xs[u] = row[v];
    sb[u] = suppress_bits ? suppress_bits[v >> 5] : 0u;
  }
#pragma unroll
  for (int u = 0; u < BP_MAXE; ++u) {
    const int v = v0 + tid + 256 * u;
    if (v < v1) visit(v, xs[u], sb[u]);
  }
  for (int v = v0 + tid + 256 * BP_MAXE; v < v1; v += 256) visit(v, row[v], suppress_bits ? suppress_bits[v >> 5] : 0u);
  BPROBE(0, 1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float m2 = __shfl_xor(m_all, o, 64), s2 = __shfl_xor(s_all, o, 64);
    lse_merge(m_all, s_all, m2, s2);
    m2 = __shfl_xor(m_ts, o, 64);
    s2 = __shfl_xor(s_ts, o, 64);
    lse_merge(m_ts, s_ts, m2, s2);
    if (renorm) {
      m2 = __shfl_xor(m_tx, o, 64);
      s2 = __shfl_xor(s_tx, o, 64);
      lse_merge(m_tx, s_tx, m2, s2);
    }
  }
  // a chunk wholly below the timestamps has no timestamp candidate (14 of the 16 chunks at large-v3 sizes), one
  // wholly inside them no text candidate: that list's K dependent argmax rounds (here and in the merge below) are
  // skipped, uniformly per block (each round is a 6-level shuffle chain: the reductions were ~20 us of 55)
  const bool any_ts = p.use_timestamps && v1 > tsb, any_tx = !p.use_timestamps || v0 < tsb;
  BPROBE(0, 2);
  if (any_tx) wave_topk<K>(T, wl[0][wid], lane);
  if (any_ts) wave_topk<K>(S, wl[1][wid], lane);
  BPROBE(0, 3);
  if (lane == 0) {
    wst[wid][0] = m_all;
    wst[wid][1] = s_all;
    wst[wid][2] = m_ts;
    wst[wid][3] = s_ts;
    wst[wid][4] = m_tx;
    wst[wid][5] = s_tx;
  }
  __syncthreads();
  if (wid != 0) return;
  BeamPart<K>* out = ws + (size_t)b * NC + c;
  for (int l = 0; l < 2; ++l) {  // merge the 4 wave lists: lane q holds entry q (4K <= 64), K rounds of argmax
    if (!(l == 0 ? any_tx : any_ts)) {  // an empty list
      if (lane < K) {
        if (l == 0) out->t[lane] = Cand{-INFINITY, 0x7fffffff};
        else out->s[lane] = Cand{-INFINITY, 0x7fffffff};
      }
      continue;
    }
    // the block's top-K of the 4 waves' lists by rank (each of the 4K entries counts the entries ahead of it under
    // the rounds' order, position breaking ties): one pass over 4K LDS broadcasts instead of K argmax rounds
    if (lane < 4 * K) {
      const Cand* all = &wl[l][0][0];
      const Cand mine = all[lane];
      int rank = 0;
      for (int e = 0; e < 4 * K; ++e) {
        const Cand o = all[e];
        rank += (o.v > mine.v) | ((o.v == mine.v) & ((o.i < mine.i) | ((o.i == mine.i) & (e < lane))));
      }
      if (rank < K) {
        if (l == 0) out->t[rank] = mine;
        else out->s[rank] = mine;
      }
    }
  }
  if (lane == 0) {
    float ma = wst[0][0], sa = wst[0][1], mt = wst[0][2], st2 = wst[0][3], mx = wst[0][4], sx = wst[0][5];
    for (int w = 1; w < 4; ++w) {
      lse_merge(ma, sa, wst[w][0], wst[w][1]);
      lse_merge(mt, st2, wst[w][2], wst[w][3]);
      lse_merge(mx, sx, wst[w][4], wst[w][5]);
    }
    out->m_all = ma;
    out->s_all = sa;
    out->m_ts = mt;
    out->s_ts = st2;
    out->m_tx = mx;
    out->s_tx = sx;
  }
  BPROBE(0, 4);
}

#define TW_BEAM_MAXNB 8
#define TW_BEAM_MAXT 448

template <int K>
__global__ __launch_bounds__(512) void k_beam_step(const BeamPart<K>* __restrict__ ws, int NC, TwSelectParams p,
                                                   TwBeamParams bp, TwBeamState bs, int* __restrict__ state,
                                                   int* __restrict__ tokens, int* __restrict__ ids,
                                                   int* __restrict__ pos) {
  TW_DEC_PRIO();
  BPROBE(1, 0);
  __shared__ Cand rc[TW_BEAM_MAXNB][K];  // row candidates: accumulated log-prob, token
  __shared__ int old_tok[TW_BEAM_MAXNB][TW_BEAM_MAXT];
  __shared__ int old_fin[TW_BEAM_MAXNB][TW_BEAM_MAXT];
  __shared__ int old_st[TW_BEAM_MAXNB][TW_STATE_STRIDE];
  __shared__ int old_tab[TW_BEAM_MAXNB][TW_BEAM_MAXT];  // the K/V position table rows (bs.kv_tab)
  __shared__ int old_ftab[TW_BEAM_MAXNB][TW_BEAM_MAXT];  // the finished hypotheses' tables (bs.fin_tab)
  __shared__ int old_pos[TW_BEAM_MAXNB];
  __shared__ int old_flen[TW_BEAM_MAXNB];
  __shared__ int s_src[TW_BEAM_MAXNB], s_tok[TW_BEAM_MAXNB], f_from[TW_BEAM_MAXNB], f_flag[TW_BEAM_MAXNB];
  __shared__ float s_score[TW_BEAM_MAXNB], f_score[TW_BEAM_MAXNB];
  // (bs.run_lp: every candidate's running sum of log-probabilities renormalised over the allowed tokens — what
  // _retrieve_avg_logprobs takes from the processed beam scores — carried beside the beam scores)
  __shared__ float rc_lp[TW_BEAM_MAXNB][K], c_lp[2 * K], s_lp[TW_BEAM_MAXNB], f_lp[TW_BEAM_MAXNB];
  // (bs.run_tlp / fin_tlp: each candidate's own term of that sum, written at position t of the per-token histories)
  __shared__ float rc_tm[TW_BEAM_MAXNB][K], c_tm[2 * K], s_tm[TW_BEAM_MAXNB];
  __shared__ int c_beam[2 * K], c_tok[2 * K];
  // per-row sorted lists and the one-thread bookkeeping arrays live in LDS: as per-thread arrays with runtime
  // indices they were lowered to scratch (224-768 B/lane) and the serial section ran at scratch latency
  __shared__ Cand tops[TW_BEAM_MAXNB][2][K];
  __shared__ float csc[2 * K], rsc[2 * K], merged[TW_BEAM_MAXNB + 2 * K];
  __shared__ bool hits[2 * K];
  const int w = blockIdx.x, nb = bp.num_beams, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ldt = bp.ld_tokens;
  const bool lpt = bs.run_lp != nullptr && bs.fin_lp != nullptr;
  const bool tlp = lpt && bs.run_tlp != nullptr && bs.fin_tlp != nullptr;
  int* win = bs.win + 4 * w;
  const int t = win[2];
  const float NEG = -1.0e9f;
  // the window's running and finished histories and processor states, loaded now so their latency hides behind
  // step 1 (as a load-then-LDS-store loop after it, each trip waited for its own loads); positions past a history's
  // length are staged too (any value: they are never read back)
  constexpr int STG = (TW_BEAM_MAXNB * TW_BEAM_MAXT + 511) / 512;
  int rt[STG], rf[STG], rk[STG], rft[STG];
  // the per-token log-probability histories stay in registers (no LDS left for two more staged arrays): every thread
  // reads its entries here, before any block-wide barrier, and in section 3 writes them to the slots that take them
  float rl[STG], rfl[STG];
  const bool tab = bs.kv_tab != nullptr;
  const bool ftab = tab && bs.fin_tab != nullptr;
#pragma unroll
  for (int u = 0; u < STG; ++u) {
    const int e = tid + 512 * u, j = e / TW_BEAM_MAXT, q = e % TW_BEAM_MAXT;
    const bool ok = j < nb && q < ldt;
    const size_t off = (size_t)(w * nb + (ok ? j : 0)) * ldt + (ok ? q : 0);
    rt[u] = ok ? tokens[off] : 0;
    rf[u] = ok ? bs.fin_tokens[off] : 0;
    rk[u] = ok && tab ? bs.kv_tab[off] : 0;
    rft[u] = ok && ftab ? bs.fin_tab[off] : 0;
    rl[u] = ok && tlp ? bs.run_tlp[off] : 0.f;
    rfl[u] = ok && tlp ? bs.fin_tlp[off] : 0.f;
  }
  const int st_v = tid < nb * TW_STATE_STRIDE ? state[(w * nb) * TW_STATE_STRIDE + tid] : 0;
  const int fl_v = tid < nb ? bs.fin_len[w * nb + tid] : 0;
  const int ps_v = tid < nb ? pos[w * nb + tid] : 0;
  BPROBE(1, 1);

  // 1. per row (one wave each): merge the chunk records, apply the timestamp rule, score the candidates
  if (wid < nb) {
    const int row = w * nb + wid;
    const BeamPart<K>* parts = ws + (size_t)row * NC;
    float m_all = -INFINITY, s_all = 0.f, m_ts = -INFINITY, s_ts = 0.f, m_tx = -INFINITY, s_tx = 0.f;
    for (int c = lane; c < NC; c += 64) {
      lse_merge(m_all, s_all, parts[c].m_all, parts[c].s_all);
      lse_merge(m_ts, s_ts, parts[c].m_ts, parts[c].s_ts);
      if (lpt) lse_merge(m_tx, s_tx, parts[c].m_tx, parts[c].s_tx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float m2 = __shfl_xor(m_all, o, 64), s2 = __shfl_xor(s_all, o, 64);
      lse_merge(m_all, s_all, m2, s2);
      m2 = __shfl_xor(m_ts, o, 64);
      s2 = __shfl_xor(s_ts, o, 64);
      lse_merge(m_ts, s_ts, m2, s2);
      if (lpt) {
        m2 = __shfl_xor(m_tx, o, 64);
        s2 = __shfl_xor(s_tx, o, 64);
        lse_merge(m_tx, s_tx, m2, s2);
      }
    }
    BPROBE(1, 8);
    // top-K of the text list and of the timestamp list over the NC chunk lists (<= 4 entries per lane). With the
    // timestamp split of k_beam_partial every timestamp candidate sits in the last chunk's (sorted) list and every
    // other chunk's list is empty: that list is the merge's result as it stands
    Cand(*top)[K] = tops[wid];
    const bool split_ts = p.use_timestamps && p.ts_begin > 0 && p.ts_begin < p.V && NC > 1;
    if (split_ts && lane < K) top[1][lane] = parts[NC - 1].s[lane];
    for (int l = 0; l < (split_ts ? 1 : 2); ++l) {
      Cand mine[4];
      bool used[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = lane + 64 * q;
        mine[q] = e < NC * K ? (l == 0 ? parts[e / K].t[e % K] : parts[e / K].s[e % K]) : Cand{-INFINITY, 0x7fffffff};
        used[q] = false;
      }
      for (int r = 0; r < K; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff, bq = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool b = !used[q] & cand_better(mine[q].v, mine[q].i, Cand{bv, bi});
          bv = b ? mine[q].v : bv;
          bi = b ? mine[q].i : bi;
          bq = b ? q : bq;
        }
        int bl = lane;
        wave_best(bv, bi, bl);
#pragma unroll
        for (int q = 0; q < 4; ++q) used[q] = used[q] || (lane == bl && bq == q);
        if (lane == 0) top[l][r] = Cand{bv, bi};
      }
      BPROBE(1, 9 + l);
    }
    if (lane == 0) {  // lane 0 wrote top
      const float lse_all = m_all + __logf(s_all);
      const float lse_ts = (m_ts == -INFINITY) ? -INFINITY : m_ts + __logf(s_ts);
      // WhisperTimeStampLogitsProcessor: timestamp mass above every text token -> text tokens -inf
      const bool fires = p.use_timestamps && lse_ts > top[0][0].v;
      const float run = bs.run_score[row];
      // the allowed set log_softmax renormalises over: the allowed timestamps alone when the rule fires
      float lse_ok = 0.f, run_lp = 0.f;
      if (lpt) {
        const float lse_tx = (m_tx == -INFINITY) ? -INFINITY : m_tx + __logf(s_tx);
        lse_ok = fires ? lse_ts : (lse_tx == -INFINITY ? lse_ts : lse_ts == -INFINITY ? lse_tx
                                   : fmaxf(lse_tx, lse_ts) + log1pf(__expf(-fabsf(lse_tx - lse_ts))));
        run_lp = bs.run_lp[row];
      }
      int a = 0, bb = 0;
      for (int k = 0; k < K; ++k) {
        Cand pick;
        if (fires) {
          pick = top[1][bb++];
        } else if (cand_better(top[0][a].v, top[0][a].i, top[1][bb])) {
          pick = top[0][a++];
        } else {
          pick = top[1][bb++];
        }
        // (bp.scores_are_logprobs: tw_logits_history already wrote log_softmax + the history processors)
        const float lp_all = bp.scores_are_logprobs ? pick.v : pick.v - lse_all;
        rc[wid][k] = Cand{pick.v == -INFINITY ? -INFINITY : run + lp_all, pick.i};
        if (lpt) rc_lp[wid][k] = pick.v == -INFINITY ? -INFINITY : run_lp + (pick.v - lse_ok);
        if (tlp) rc_tm[wid][k] = pick.v == -INFINITY ? -INFINITY : pick.v - lse_ok;
      }
    }
  }
  BPROBE(1, 11);
  // stage the old running histories, finished histories and processor states of the window
#pragma unroll
  for (int u = 0; u < STG; ++u) {
    const int e = tid + 512 * u, j = e / TW_BEAM_MAXT, q = e % TW_BEAM_MAXT;
    if (j < nb) {
      old_tok[j][q] = rt[u];
      old_fin[j][q] = rf[u];
      old_tab[j][q] = rk[u];
      old_ftab[j][q] = rft[u];
    }
  }
  if (tid < nb * TW_STATE_STRIDE) old_st[tid / TW_STATE_STRIDE][tid % TW_STATE_STRIDE] = st_v;
  if (tid < nb) {
    old_flen[tid] = fl_v;
    old_pos[tid] = ps_v;
  }
  BPROBE(1, 2);
  __syncthreads();
  BPROBE(1, 3);

  // 2. the window's beam bookkeeping. Each selection below is a stable top-n; it is computed as ranks, every
  // candidate counting the candidates ahead of it (LDS broadcast reads), instead of n sequential argmax rounds in
  // one thread (that serial section was ~25 of the kernel's 52 us at 12 windows x 5 beams).
  // a. top-K over all beams' candidates by accumulated log-prob; ties -> lower flat index beam * V + token (rows
  //    hold distinct tokens; a row's repeated empty entries keep their list order)
  if (tid < nb * K) {
    const int j = tid / K, k = tid - j * K;
    const float v = rc[j][k].v;
    const long f = (long)j * p.V + rc[j][k].i;
    int rank = 0;
    for (int e = 0; e < nb * K; ++e) {
      const int j2 = e / K, k2 = e - j2 * K;
      const float v2 = rc[j2][k2].v;
      const long f2 = (long)j2 * p.V + rc[j2][k2].i;
      rank += (v2 > v) | ((v2 == v) & ((f2 < f) | ((f2 == f) & (e < tid))));  // (bitwise: no branches)
    }
    if (rank < K) {
      c_beam[rank] = j;
      c_tok[rank] = rc[j][k].i;
      csc[rank] = v;
      if (lpt) c_lp[rank] = rc_lp[j][k];
      if (tlp) c_tm[rank] = rc_tm[j][k];
    }
  }
  __syncthreads();
  BPROBE(1, 4);
  const int unsat_prev = win[0];
  const float lp_div = __powf((float)(t + 1), bp.length_penalty);
  if (tid < K) {
    const int c = tid;
    hits[c] = c_tok[c] == p.eos || t + 1 >= bp.max_new;
    rsc[c] = csc[c] + (hits[c] ? NEG : 0.f);
  }
  // f. the finished candidates: previous best nb, then the just-finished top-nb continuations
  if (tid < nb + K) {
    const int e = tid;
    if (e < nb) {
      merged[e] = bs.fin_score[w * nb + e];
    } else {
      const int c = e - nb;
      float v = csc[c] / lp_div;
      if (!unsat_prev) v += NEG;
      const bool just = (c_tok[c] == p.eos || t + 1 >= bp.max_new) && c < nb;
      if (!just) v += NEG;
      merged[e] = v;
    }
  }
  __syncthreads();
  // e. running beams for the next step: best nb of the continuations by rsc (ties -> lower c)
  if (tid < K) {
    const int c = tid;
    int rank = 0;
    for (int c2 = 0; c2 < K; ++c2) rank += (rsc[c2] > rsc[c]) | ((rsc[c2] == rsc[c]) & (c2 < c));
    if (rank < nb) {
      s_src[rank] = c_beam[c];
      s_tok[rank] = c_tok[c];
      s_score[rank] = rsc[c];
      if (lpt) s_lp[rank] = c_lp[c];
      if (tlp) s_tm[rank] = c_tm[c];
    }
  }
  // f. finished beams: best nb of the nb + K merged scores (ties -> lower e)
  if (tid >= 64 && tid < 64 + nb + K) {
    const int e = tid - 64;
    int rank = 0;
    for (int e2 = 0; e2 < nb + K; ++e2) rank += (merged[e2] > merged[e]) | ((merged[e2] == merged[e]) & (e2 < e));
    if (rank < nb) {
      f_from[rank] = e;
      f_score[rank] = merged[e];
      f_flag[rank] = e < nb ? bs.fin_flag[w * nb + e] : (hits[e - nb] && e - nb < nb);
      if (lpt) f_lp[rank] = e < nb ? bs.fin_lp[w * nb + e] : c_lp[e - nb];
    }
  }
  __syncthreads();
  // g. early-stop heuristic (early_stopping=False: best running score at the current length)
  if (tid == 0) {
    bool all_hit = true;
    for (int c = 0; c < K; ++c) all_hit = all_hit && hits[c];
    float min_fin = INFINITY;
    for (int q = 0; q < nb; ++q) min_fin = fminf(min_fin, f_score[q]);
    const float best_possible = s_score[0] / __powf((float)(t + 1), bp.length_penalty);
    bool any_better = false;
    for (int q = 0; q < nb; ++q) any_better = any_better || best_possible > (f_flag[q] ? min_fin : NEG);
    const int unsat = unsat_prev && any_better;
    win[0] = unsat;
    win[1] = (!unsat || all_hit) ? 1 : 0;
    win[2] = t + 1;
  }
  __syncthreads();
  BPROBE(1, 5);

  // 3. apply: running histories, state, ids, pos, the K/V source rows; finished histories
  for (int e = tid; e < nb * (t + 1); e += blockDim.x) {
    const int j = e / (t + 1), q = e % (t + 1);
    tokens[(size_t)(w * nb + j) * ldt + q] = q < t ? old_tok[s_src[j]][q] : s_tok[j];
  }
  // K/V position table: the new beam j reads its source's history, positions [0, pos + 1) (this step's position
  // included: the source wrote it); later positions keep j's own row (kv_tab[r][*] = r from the pass start)
  if (tab) {
    for (int e = tid; e < nb * TW_BEAM_MAXT; e += blockDim.x) {
      const int j = e / TW_BEAM_MAXT, q = e % TW_BEAM_MAXT;
      if (q <= old_pos[j] && q < ldt && s_src[j] != j) bs.kv_tab[(size_t)(w * nb + j) * ldt + q] = old_tab[s_src[j]][q];
    }
  }
  for (int e = tid; e < nb * TW_BEAM_MAXT; e += blockDim.x) {
    const int qs = e / TW_BEAM_MAXT, q = e % TW_BEAM_MAXT;
    const int from = f_from[qs];
    int len, v;
    if (from < nb) {
      len = old_flen[from];
      v = q < len ? old_fin[from][q] : 0;
    } else {
      const int c = from - nb;
      len = t + 1;
      v = q < t ? old_tok[c_beam[c]][q] : c_tok[c];
    }
    if (q < len) bs.fin_tokens[(size_t)(w * nb + qs) * ldt + q] = v;
    // the rows that fed the history's positions: a kept slot's own table, or (just finished) its source beam's
    // table up to the position the source fed this step
    if (ftab && q < ldt) {
      int r;
      if (from < nb) {
        r = old_ftab[from][q];
      } else {
        const int src = c_beam[from - nb];
        r = q <= old_pos[src] ? old_tab[src][q] : 0;
      }
      bs.fin_tab[(size_t)(w * nb + qs) * ldt + q] = r;
    }
  }
  // the per-token log-probabilities move as tokens / fin_tokens do: positions [0, t) of a source's history (held in
  // this thread's registers since the kernel's start) go to every slot that continues or keeps it, position t takes
  // the continuation's own term
  if (tlp) {
#pragma unroll
    for (int u = 0; u < STG; ++u) {
      const int e = tid + 512 * u, j = e / TW_BEAM_MAXT, q = e % TW_BEAM_MAXT;
      if (j >= nb || q >= ldt) continue;
      for (int d = 0; d < nb; ++d) {
        const size_t off = (size_t)(w * nb + d) * ldt + q;
        if (s_src[d] == j && q < t) bs.run_tlp[off] = rl[u];
        const int from = f_from[d];
        if (from < nb) {
          if (from == j && q < old_flen[j]) bs.fin_tlp[off] = rfl[u];
        } else if (c_beam[from - nb] == j && q < t) {
          bs.fin_tlp[off] = rl[u];
        }
      }
    }
    if (tid < nb && t < ldt) {
      const size_t off = (size_t)(w * nb + tid) * ldt + t;
      bs.run_tlp[off] = s_tm[tid];
      if (f_from[tid] >= nb) bs.fin_tlp[off] = c_tm[f_from[tid] - nb];
    }
  }
  if (tid < nb) {
    const int j = tid, row = w * nb + j, src = s_src[j], tok = s_tok[j];
    int* st = state + row * TW_STATE_STRIDE;
    st[TW_ST_NGEN] = t + 1;
    st[TW_ST_PENULT] = old_st[src][TW_ST_LAST];
    st[TW_ST_LAST] = tok;
    st[TW_ST_LASTTS] = (p.use_timestamps && tok >= p.ts_begin) ? tok : old_st[src][TW_ST_LASTTS];
    st[TW_ST_FINISHED] = 0;
    ids[row] = tok;
    pos[row] += 1;
    bs.src_rows[row] = w * nb + src;
    bs.run_score[row] = s_score[j];
    const int from = f_from[j];
    bs.fin_score[row] = f_score[j];
    bs.fin_flag[row] = f_flag[j];
    bs.fin_len[row] = from < nb ? old_flen[from] : t + 1;
    if (lpt) {
      bs.run_lp[row] = s_lp[j];
      bs.fin_lp[row] = f_lp[j];
    }
  }
  BPROBE(1, 6);
}

template <int K>
static int launch_beam(const float* logits, int W, int ld_logits, const uint32_t* suppress_bits,
                       const TwSelectParams* p, const TwBeamParams* bp, TwBeamState bs, int* state, int* tokens,
                       int* ids, int* pos, void* workspace, hipStream_t s) {
  const int R = W * bp->num_beams;
  BeamPart<K>* ws = (BeamPart<K>*)workspace;
  hipLaunchKernelGGL(k_beam_partial<K>, dim3(R, TW_SELECT_CHUNKS), dim3(256), 0, s, logits, ld_logits, suppress_bits,
                     *p, state, ws, (int)(bs.run_lp != nullptr && bs.fin_lp != nullptr));
  hipLaunchKernelGGL(k_beam_step<K>, dim3(W), dim3(512), 0, s, ws, TW_SELECT_CHUNKS, *p, *bp, bs, state, tokens, ids,
                     pos);
  return tw_check_launch("tw_beam_step");
}

extern "C" size_t tw_beam_workspace_bytes(int rows) {
  return (size_t)rows * TW_SELECT_CHUNKS * sizeof(BeamPart<2 * TW_BEAM_MAXNB>);
}

extern "C" int tw_beam_step(const float* logits, int W, int ld_logits, const uint32_t* suppress_bits,
                            const TwSelectParams* params, const TwBeamParams* bp, const TwBeamState* bs, int* state,
                            int* tokens, int* ids, int* pos, void* workspace, void* stream) {
  TW_REQUIRE(logits && params && bp && bs && state && tokens && ids && pos && workspace && W > 0,
             "tw_beam_step: null argument");
  TW_REQUIRE(bp->num_beams >= 2 && bp->num_beams <= TW_BEAM_MAXNB, "tw_beam_step: num_beams=%d (2..%d)",
             bp->num_beams, TW_BEAM_MAXNB);
  TW_REQUIRE(bp->ld_tokens <= TW_BEAM_MAXT && bp->max_new >= 1 && bp->max_new <= bp->ld_tokens,
             "tw_beam_step: ld_tokens=%d max_new=%d", bp->ld_tokens, bp->max_new);
  TW_REQUIRE(params->mode == 0 && params->V <= ld_logits, "tw_beam_step: params");
  hipStream_t s = (hipStream_t)stream;
  switch (bp->num_beams) {
    case 2: return launch_beam<4>(logits, W, ld_logits, suppress_bits, params, bp, *bs, state, tokens, ids, pos, workspace, s);
    case 3: return launch_beam<6>(logits, W, ld_logits, suppress_bits, params, bp, *bs, state, tokens, ids, pos, workspace, s);
    case 4: return launch_beam<8>(logits, W, ld_logits, suppress_bits, params, bp, *bs, state, tokens, ids, pos, workspace, s);
    case 5: return launch_beam<10>(logits, W, ld_logits, suppress_bits, params, bp, *bs, state, tokens, ids, pos, workspace, s);
    case 6: return launch_beam<12>(logits, W, ld_logits, suppress_bits, params, bp, *bs, state, tokens, ids, pos, workspace, s);
    case 7: return launch_beam<14>(logits, W, ld_logits, suppress_bits, params, bp, *bs, state, tokens, ids, pos, workspace, s);
    default: return launch_beam<16>(logits, W, ld_logits, suppress_bits, params, bp, *bs, state, tokens, ids, pos, workspace, s);
  }
}

// =================================================================================================
// Token alternatives: the k best eligible ids of a step's processed scores with their log-probabilities, in front of
// the selection on the same logits, params and (only read) state.
//   k_beam_partial<TW_TOPK_MAX>, renorm = 1   grid (B, NC): per chunk the top-8 masked text and timestamp candidates
//                   and the logsumexp states of the allowed text / timestamp tokens (a workspace of its own)
//   k_topk_final    grid B, one wave per row: merges the NC records, decides the timestamp rule as the selection does
//                   (sel_rule_fires), and takes the top k of what is left under cand_better's order
// A candidate list can hold ids whose score is -inf without a mask (a history processor wrote it): they are not
// eligible and become sentinels here.
// =================================================================================================
__global__ __launch_bounds__(64) void k_topk_final(const BeamPart<TW_TOPK_MAX>* __restrict__ ws, int NC,
                                                   TwSelectParams p, const int* __restrict__ state, int k,
                                                   int32_t* __restrict__ ids_out, float* __restrict__ lp_out,
                                                   int ld_out) {
  TW_DEC_PRIO();
  constexpr int K = TW_TOPK_MAX;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* st = state + b * TW_STATE_STRIDE;
  const int q = st[TW_ST_NGEN];
  if (q < 0 || q >= ld_out) return;  // (uniform per block)
  const size_t o = ((size_t)b * ld_out + q) * k;
  if (st[TW_ST_FINISHED]) {
    if (lane < k) {
      ids_out[o + lane] = -1;
      lp_out[o + lane] = -INFINITY;
    }
    return;
  }
  const BeamPart<K>* parts = ws + (size_t)b * NC;
  // the pool: NC * K text and NC * K timestamp candidates, lane l holds entries l and l + 64 of each list
  // (NC * K <= 128); static indices only, so it stays in registers
  Cand pool[4];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = lane + 64 * u;
    const bool ok = e < NC * K;
    pool[u] = ok ? parts[e / K].t[e % K] : Cand{-INFINITY, 0x7fffffff};
    pool[2 + u] = ok ? parts[e / K].s[e % K] : Cand{-INFINITY, 0x7fffffff};
  }
  float m_ts = -INFINITY, s_ts = 0.f, m_tx = -INFINITY, s_tx = 0.f;
  for (int c = lane; c < NC; c += 64) {
    lse_merge(m_ts, s_ts, parts[c].m_ts, parts[c].s_ts);
    lse_merge(m_tx, s_tx, parts[c].m_tx, parts[c].s_tx);
  }
#pragma unroll
  for (int x = 32; x > 0; x >>= 1) {
    float m2 = __shfl_xor(m_ts, x, 64), s2 = __shfl_xor(s_ts, x, 64);
    lse_merge(m_ts, s_ts, m2, s2);
    m2 = __shfl_xor(m_tx, x, 64);
    s2 = __shfl_xor(s_tx, x, 64);
    lse_merge(m_tx, s_tx, m2, s2);
  }
  // the best text candidate decides the rule
  Cand bt = cand_better(pool[1].v, pool[1].i, pool[0]) ? pool[1] : pool[0];
  {
    int bl = lane;
    wave_best(bt.v, bt.i, bl);
  }
  const bool fire = sel_rule_fires(p, Best{bt.v, bt.i}, m_ts, s_ts);
  float m = fire ? -INFINITY : m_tx, sm = fire ? 0.f : s_tx;
  if (p.use_timestamps) lse_merge(m, sm, m_ts, s_ts);
  const float lse = m + __logf(sm);
  if (fire) pool[0] = pool[1] = Cand{-INFINITY, 0x7fffffff};
  // k rounds of wave argmax over the pool; lane r keeps round r's winner
  Cand mine{-INFINITY, 0x7fffffff};
  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY;
    int bi = 0x7fffffff, bq = -1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool better = cand_better(pool[u].v, pool[u].i, Cand{bv, bi});
      bv = better ? pool[u].v : bv;
      bi = better ? pool[u].i : bi;
      bq = better ? u : bq;
    }
    int bl = lane;
    wave_best(bv, bi, bl);
    const bool won = lane == bl;
#pragma unroll
    for (int u = 0; u < 4; ++u) pool[u] = (won & (bq == u)) ? Cand{-INFINITY, 0x7fffffff} : pool[u];
    if (lane == r) mine = Cand{bv, bi};
  }
  if (lane < k) {
    const bool has = mine.v != -INFINITY;
    ids_out[o + lane] = has ? mine.i : -1;
    lp_out[o + lane] = has ? mine.v - lse : -INFINITY;
  }
}

extern "C" size_t tw_token_topk_workspace_bytes(int rows) {
  return (size_t)(rows > 0 ? rows : 0) * TW_SELECT_CHUNKS * sizeof(BeamPart<TW_TOPK_MAX>);
}

extern "C" int tw_token_topk(const float* logits, int B, int ld_logits, const uint32_t* suppress_bits,
                             const TwSelectParams* params, const int* state, int k, int32_t* ids_out, float* lp_out,
                             int ld_out, void* workspace, void* stream) {
  TW_REQUIRE(logits && params && state && ids_out && lp_out && workspace && B > 0 && ld_out > 0,
             "tw_token_topk: bad args");
  TW_REQUIRE(k >= 1 && k <= TW_TOPK_MAX, "tw_token_topk: k=%d (1..%d)", k, TW_TOPK_MAX);
  TW_REQUIRE(params->mode == 0, "tw_token_topk: generation steps (mode 0) only");
  TW_REQUIRE(params->V > 0 && params->V <= ld_logits, "tw_token_topk: V=%d ld=%d", params->V, ld_logits);
  TW_REQUIRE(params->n_begin_suppress >= 0 && params->n_begin_suppress <= 8, "tw_token_topk: begin_suppress");
  static_assert(TW_SELECT_CHUNKS * TW_TOPK_MAX <= 128, "k_topk_final: two entries of each list per lane");
  hipStream_t s = (hipStream_t)stream;
  BeamPart<TW_TOPK_MAX>* ws = (BeamPart<TW_TOPK_MAX>*)workspace;
  hipLaunchKernelGGL(k_beam_partial<TW_TOPK_MAX>, dim3(B, TW_SELECT_CHUNKS), dim3(256), 0, s, logits, ld_logits,
                     suppress_bits, *params, state, ws, 1);
  hipLaunchKernelGGL(k_topk_final, dim3(B), dim3(64), 0, s, ws, TW_SELECT_CHUNKS, *params, state, k, ids_out, lp_out,
                     ld_out);
  return tw_check_launch("tw_token_topk");
}

// Self-attention K/V reorder after a beam step: row r continues row src_rows[r]; positions [0, pos[r]) move.
// In place, one launch for K and V: block (layer*head, position tile, K|V) stages the tile of every moved row's
// source in LDS, then writes the destinations. Tiles are disjoint across blocks and a block reads all its sources
// before it writes, so any permutation is safe; HBM traffic is one read + one write per moved (row, position)
// (the earlier two-phase copy through a cache-sized scratch moved every byte twice, in four launches).
#define TW_KVR_LDS 57344
__global__ __launch_bounds__(256) void k_kv_reorder(bf16_t* __restrict__ k_cache, bf16_t* __restrict__ v_cache,
                                                    const int* __restrict__ src_rows, const int* __restrict__ pos,
                                                    int rows_cap, int H, int T, int R, int TT) {
  extern __shared__ uint4 kvr_tile[];  // [R][TT * 8] uint4 (a position of one head = 64 bf16 = 8 uint4)
  __shared__ int s_src[512], s_n[512];
  __shared__ int s_any;
  const int lh = blockIdx.x, l = lh / H, h = lh - l * H, t0 = blockIdx.y * TT;
  bf16_t* cache = blockIdx.z == 0 ? k_cache : v_cache;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += 256) {
    const int s = src_rows[r];
    // positions of this tile row r takes from s (an out-of-range source or position moves nothing: never a fault)
    const bool ok = s != r && s >= 0 && s < rows_cap;
    const int n = ok ? min(max(min(pos[r], T) - t0, 0), TT) : 0;
    s_src[r] = s;
    s_n[r] = n;
    if (n > 0) s_any = 1;
  }
  __syncthreads();
  if (!s_any) return;
  const int per_row = TT * 8;
  const size_t head = (size_t)T * 8;  // uint4 per (layer, row, head)
  const uint4* c4 = (const uint4*)cache;
  for (int e = threadIdx.x; e < R * per_row; e += 256) {
    const int r = e / per_row, q = e - r * per_row;
    if (q < s_n[r] * 8)
      kvr_tile[e] = c4[(((size_t)l * rows_cap + s_src[r]) * H + h) * head + (size_t)t0 * 8 + q];
  }
  __syncthreads();
  uint4* w4 = (uint4*)cache;
  for (int e = threadIdx.x; e < R * per_row; e += 256) {
    const int r = e / per_row, q = e - r * per_row;
    if (q < s_n[r] * 8) w4[(((size_t)l * rows_cap + r) * H + h) * head + (size_t)t0 * 8 + q] = kvr_tile[e];
  }
}

extern "C" int tw_kv_reorder(uint16_t* k_cache, uint16_t* v_cache, uint16_t* k_scratch, uint16_t* v_scratch, int layers,
                             int rows_cap, int H, int T, int R, const int* src_rows, const int* pos, void* stream) {
  (void)k_scratch;
  (void)v_scratch;
  // one position per tile at least: R * 128 B of dynamic LDS within TW_KVR_LDS (R <= 448)
  TW_REQUIRE(k_cache && v_cache && src_rows && pos && R > 0 && R <= rows_cap && R <= TW_KVR_LDS / 128 && T > 0,
             "tw_kv_reorder: bad args (R=%d rows_cap=%d T=%d; R <= %d)", R, rows_cap, T, TW_KVR_LDS / 128);
  int TT = 16;  // positions per tile: R * TT * 128 B of LDS
  while (TT > 1 && (size_t)R * TT * 128 > TW_KVR_LDS) TT >>= 1;
  const dim3 grid(layers * H, (T + TT - 1) / TT, 2);
  hipLaunchKernelGGL(k_kv_reorder, grid, dim3(256), (size_t)R * TT * 128, (hipStream_t)stream, (bf16_t*)k_cache,
                     (bf16_t*)v_cache, src_rows, pos, rows_cap, H, T, R, TT);
  return tw_check_launch("tw_kv_reorder");
}
