// Forced alignment: the alignment heads' recorded cross-attention -> the DTW cost matrix, on the device.
//
// The host path (twamd/alignment.py token_timestamps, WhisperGenerationMixin._extract_token_timestamps,
// $TF/models/whisper/generation_whisper.py:241-380) copies probs f32[B][n_steps][n_slots][S] to the host and runs,
// per row: standardise every (slot, frame) column over the tokens, median-filter each (slot, token) row over the
// frames (reflect padding, the middle of the sorted window, NaN last), average the slots, negate. This kernel does the
// same per row b over that row's own n_rows[b] tokens and n_frames[b] frames and writes cost f32[B][n_steps][S]:
// the probabilities are read twice (statistics, then values) and 1 / n_slots of their size is written.
//
// One workgroup of ALN_T threads per (frame tile, row): thread t owns column f0 - pad + t (reflected at the crop's
// edges), so a tile is ALN_T - 2 pad output frames plus its halo, and every token-loop load is one coalesced run.
//   phase 1  per slot, mean and population deviation of the column over the tokens, as numpy's mean / std: the sum,
//            then the sum of squared deviations from the mean (eight partial sums each, the eight loads of a trip in
//            flight together; the second pass re-reads a block of n_rows x 512 B the first just brought into the
//            L2). A column of identical values has mean == value and deviation == 0 exactly, so its z is NaN as in
//            float64, whatever the f32 sum of the values rounds to. Kept in LDS for the tile and its halo;
//   phase 2  per token: every thread standardises its column's value of each slot into LDS (as order-preserving
//            integer keys, NaN largest), then the threads of the tile's interior sort their 2 pad + 1 neighbours in
//            registers (odd-even transposition network on the keys), take the middle, sum the slots and store.
// The next token's values are loaded before the barrier, so two tokens' loads are in flight per thread.
// Slots go through in chunks of ALN_SC (LDS and registers are sized for a chunk); a later chunk adds to the
// partial sums the same thread stored for the earlier ones.
#include "tw_common.h"
#include "../../include/tw_whisper.h"

#define ALN_T 128     // threads per workgroup = columns per tile, halo included
#define ALN_SC 8      // slots per chunk
#define ALN_KU 8      // tokens loaded per trip of the statistics loop
#define ALN_MAXW 15   // widest median window

// float -> key with the order of numpy / torch sort: ascending values, then NaN (either sign)
__device__ inline uint32_t aln_key(float z) { return z != z ? 0xffffffffu : f32_order_key(z); }

template <int WIDTH>
__global__ __launch_bounds__(ALN_T) void k_align_cost(const float* __restrict__ probs, int n_steps, int n_slots,
                                                      int S, const int* __restrict__ n_rows,
                                                      const int* __restrict__ n_frames, float* __restrict__ cost) {
  constexpr int PAD = WIDTH / 2, TF = ALN_T - 2 * PAD;
  __shared__ float s_mean[ALN_SC][ALN_T];
  __shared__ float s_std[ALN_SC][ALN_T];
  __shared__ uint32_t s_key[ALN_SC][ALN_T];
  const int b = blockIdx.y, t = threadIdx.x, f0 = blockIdx.x * TF;
  const int nr = min(n_rows[b], n_steps), nf = min(n_frames[b], S);
  if (nr < 2 || nf < 1 || f0 >= nf) return;  // (uniform per block)
  const bool filt = nf > PAD;                // a crop of <= pad frames is not filtered (and has no reflection)
  // this thread's column: frame c of the padded row, read at its reflection
  const int c = f0 - PAD + t;
  int col = c < 0 ? -c : (c >= nf ? 2 * (nf - 1) - c : c);
  const bool active = filt ? (c >= -PAD && c < nf + PAD) : (c >= 0 && c < nf);
  if (!active) col = 0;
  const bool writes = t >= PAD && t < PAD + TF && c < nf;  // (c >= 0 follows from t >= PAD)
  const size_t step_stride = (size_t)n_slots * S;
  const float* prow = probs + (size_t)b * n_steps * step_stride + col;
  float* crow = cost + (size_t)b * n_steps * S + (writes ? c : 0);

  for (int s0 = 0; s0 < n_slots; s0 += ALN_SC) {
    const int ns = min(ALN_SC, n_slots - s0);
    const bool first = s0 == 0, last = s0 + ALN_SC >= n_slots;
    // ---- phase 1: column statistics of the chunk's slots
    for (int s = 0; s < ns; ++s) {
      const float* p = prow + (size_t)(s0 + s) * S;
      float a[ALN_KU], lo = INFINITY, hi = -INFINITY;
#pragma unroll
      for (int i = 0; i < ALN_KU; ++i) a[i] = 0.f;
      for (int k0 = 0; k0 < nr; k0 += ALN_KU) {
        float x[ALN_KU];
#pragma unroll
        for (int i = 0; i < ALN_KU; ++i) x[i] = p[(size_t)min(k0 + i, nr - 1) * step_stride];
#pragma unroll
        for (int i = 0; i < ALN_KU; ++i) {
          if (k0 + i < nr) {
            a[i] += x[i];
            lo = fminf(lo, x[i]);
            hi = fmaxf(hi, x[i]);
          }
        }
      }
      // (identical values: their mean is the value itself, whatever their f32 sum rounds to)
      const float mean = lo == hi ? lo : (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) / (float)nr;
#pragma unroll
      for (int i = 0; i < ALN_KU; ++i) a[i] = 0.f;
      for (int k0 = 0; k0 < nr; k0 += ALN_KU) {  // (the column block was just read: this pass is served by the L2)
        float x[ALN_KU];
#pragma unroll
        for (int i = 0; i < ALN_KU; ++i) x[i] = p[(size_t)min(k0 + i, nr - 1) * step_stride];
#pragma unroll
        for (int i = 0; i < ALN_KU; ++i) {
          const float d = x[i] - mean;
          if (k0 + i < nr) a[i] += d * d;
        }
      }
      s_mean[s][t] = mean;
      s_std[s][t] = sqrtf((((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) / (float)nr);
    }
    // (each thread reads back only its own statistics: no barrier needed before phase 2)
    float mean[ALN_SC], sd[ALN_SC], cur[ALN_SC], nxt[ALN_SC];
#pragma unroll
    for (int s = 0; s < ALN_SC; ++s) {
      mean[s] = s < ns ? s_mean[s][t] : 0.f;
      sd[s] = s < ns ? s_std[s][t] : 1.f;
      cur[s] = s < ns ? prow[(size_t)(s0 + s) * S] : 0.f;
      nxt[s] = 0.f;
    }
    // ---- phase 2: per token, standardise, median over the frames, sum the slots
    for (int k = 0; k < nr; ++k) {
#pragma unroll
      for (int s = 0; s < ALN_SC; ++s)
        if (s < ns) s_key[s][t] = aln_key((cur[s] - mean[s]) / sd[s]);
      if (k + 1 < nr) {
#pragma unroll
        for (int s = 0; s < ALN_SC; ++s)
          if (s < ns) nxt[s] = prow[(size_t)(k + 1) * step_stride + (size_t)(s0 + s) * S];
      }
      __syncthreads();
      if (writes) {
        float acc = first ? 0.f : crow[(size_t)k * S];
        for (int s = 0; s < ns; ++s) {
          uint32_t w[WIDTH];
          if (filt) {
#pragma unroll
            for (int i = 0; i < WIDTH; ++i) w[i] = s_key[s][t - PAD + i];
#pragma unroll
            for (int pass = 0; pass < WIDTH; ++pass) {
#pragma unroll
              for (int i = pass & 1; i + 1 < WIDTH; i += 2) {
                const uint32_t lo = min(w[i], w[i + 1]), hi = max(w[i], w[i + 1]);
                w[i] = lo;
                w[i + 1] = hi;
              }
            }
          } else {
            w[PAD] = s_key[s][t];
          }
          acc += f32_from_order_key(w[PAD]);
        }
        crow[(size_t)k * S] = last ? -(acc / (float)n_slots) : acc;
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < ALN_SC; ++s) cur[s] = nxt[s];
    }
  }
}

template <int WIDTH>
static void launch_align(const float* probs, int B, int n_steps, int n_slots, int S, const int* n_rows,
                         const int* n_frames, float* cost, hipStream_t st) {
  constexpr int TF = ALN_T - 2 * (WIDTH / 2);
  hipLaunchKernelGGL(k_align_cost<WIDTH>, dim3(tw_cdiv(S, TF), B), dim3(ALN_T), 0, st, probs, n_steps, n_slots, S,
                     n_rows, n_frames, cost);
}

extern "C" int tw_align_cost(const float* probs, int B, int n_steps, int n_slots, int S, const int* n_rows,
                             const int* n_frames, int width, float* cost, void* stream) {
  TW_REQUIRE(probs && n_rows && n_frames && cost, "tw_align_cost: null pointer");
  TW_REQUIRE(B > 0 && B <= 65535 && n_steps > 0 && n_slots > 0 && S > 0, "tw_align_cost: B=%d n_steps=%d n_slots=%d "
             "S=%d", B, n_steps, n_slots, S);
  TW_REQUIRE(width >= 1 && width <= ALN_MAXW && (width & 1), "tw_align_cost: median width %d (odd, 1..%d)", width,
             ALN_MAXW);
  hipStream_t st = (hipStream_t)stream;
  switch (width) {
    case 1: launch_align<1>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
    case 3: launch_align<3>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
    case 5: launch_align<5>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
    case 7: launch_align<7>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
    case 9: launch_align<9>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
    case 11: launch_align<11>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
    case 13: launch_align<13>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
    default: launch_align<15>(probs, B, n_steps, n_slots, S, n_rows, n_frames, cost, st); break;
  }
  return tw_check_launch("tw_align_cost");
}
