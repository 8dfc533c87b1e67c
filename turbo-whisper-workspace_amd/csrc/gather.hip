// tw_gather_windows (include/tw_audio.h): one launch builds an engine batch's waveform rows out of the call's arena,
// the 16 kHz mono f32 waveforms of every input of the call, concatenated in device memory:
//     out[j][i] = i < length[j] ? arena[start[j] + i] : 0        0 <= j < rows, 0 <= i < row_len
// It replaces the copy_ + zero_ pair per window (2 B launches per batch) of the device path.
//
// A pure copy: no LDS, no reuse, one read and one write per element (24 x 480000 f32: 46 MB each way). Blocks go
// over (row chunk, row); the grid is capped at GW_MAX_BLOCKS and strides over the rest of the row. The rows' starts
// and lengths travel as kernel arguments (GW_ROWS rows per launch), so the call allocates and copies nothing.
// Every lane owns 4 consecutive floats and stores them as one 16-byte word when every out row is 16-byte aligned
// (out itself and out_stride * 4 both multiples of 16; decided on the host, per call). The source alignment differs
// per row (start[j] is any sample): a row whose arena + start[j] is 16-byte aligned loads 16-byte words, the others
// take four dword loads per lane (the four together read every cache line of the row once). A 16-byte load is taken
// only where all four elements are inside [start[j], start[j] + length[j]); the row's last partial word and the
// zero tail never touch the arena.
#include "tw_common.h"
#include "../../include/tw_audio.h"

namespace {

constexpr int GW_BLOCK = 256;
constexpr int GW_ROWS = 64;         // rows per launch (their starts / lengths are 768 bytes of kernel arguments)
constexpr int GW_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks

struct GatherRows {
  int64_t start[GW_ROWS];
  int32_t length[GW_ROWS];
};

template <bool VEC_OUT>
__global__ __launch_bounds__(GW_BLOCK) void k_gather_windows(const float* __restrict__ arena, GatherRows rows,
                                                             long row_len, float* __restrict__ out, long out_stride) {
  const int j = blockIdx.y;
  const long n = rows.length[j];
  const float* __restrict__ src = arena + rows.start[j];
  float* __restrict__ dst = out + (long)j * out_stride;
  const bool vec_in = (reinterpret_cast<uintptr_t>(src) & 15) == 0;  // wave-uniform: one row per block
  const long step = (long)gridDim.x * GW_BLOCK * 4;
  for (long i = ((long)blockIdx.x * GW_BLOCK + threadIdx.x) * 4; i < row_len; i += step) {
    float4 v;
    if (vec_in && i + 4 <= n) {
      v = *reinterpret_cast<const float4*>(src + i);
    } else {
      v.x = i < n ? src[i] : 0.f;
      v.y = i + 1 < n ? src[i + 1] : 0.f;
      v.z = i + 2 < n ? src[i + 2] : 0.f;
      v.w = i + 3 < n ? src[i + 3] : 0.f;
    }
    if (VEC_OUT && i + 4 <= row_len) {
      *reinterpret_cast<float4*>(dst + i) = v;
    } else {  // an unaligned out, or the last partial word of a row_len that is no multiple of 4
      dst[i] = v.x;
      if (i + 1 < row_len) dst[i + 1] = v.y;
      if (i + 2 < row_len) dst[i + 2] = v.z;
      if (i + 3 < row_len) dst[i + 3] = v.w;
    }
  }
}

}  // namespace

extern "C" int tw_gather_windows(const float* arena, int64_t arena_len, const int64_t* start, const int32_t* length,
                                 int32_t rows, int64_t row_len, float* out, int64_t out_stride, void* stream) {
  const char* name = "tw_gather_windows";
  TW_REQUIRE(rows >= 0, "%s: rows = %d is negative", name, (int)rows);
  TW_REQUIRE(arena_len >= 0 && row_len >= 0, "%s: negative arena_len or row_len", name);
  TW_REQUIRE(row_len <= out_stride, "%s: row_len %lld exceeds out_stride %lld", name, (long long)row_len,
             (long long)out_stride);
  TW_REQUIRE(rows == 0 || (start && length), "%s: null start / length", name);
  bool any = false;
  for (int32_t j = 0; j < rows; j++) {  // every row of the call, before the first launch
    TW_REQUIRE(length[j] >= 0 && (int64_t)length[j] <= row_len, "%s: row %d: length %d is not in [0, row_len = %lld]",
               name, (int)j, (int)length[j], (long long)row_len);
    TW_REQUIRE(start[j] >= 0, "%s: row %d: start %lld is negative", name, (int)j, (long long)start[j]);
    TW_REQUIRE(start[j] <= arena_len - (int64_t)length[j], "%s: row %d: start %lld + length %d exceeds arena_len %lld",
               name, (int)j, (long long)start[j], (int)length[j], (long long)arena_len);
    any = any || length[j] > 0;
  }
  if (rows == 0 || row_len == 0) return 0;
  TW_REQUIRE(out && (arena || !any), "%s: null pointer", name);
  TW_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(arena) & 3) == 0,
             "%s: arena / out are not 4-byte aligned", name);
  const bool vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && out_stride % 4 == 0;
  hipStream_t s = (hipStream_t)stream;
  for (int32_t r0 = 0; r0 < rows; r0 += GW_ROWS) {
    const int nr = rows - r0 < GW_ROWS ? rows - r0 : GW_ROWS;
    GatherRows g;
    for (int j = 0; j < GW_ROWS; j++) {
      g.start[j] = j < nr ? start[r0 + j] : 0;
      g.length[j] = j < nr ? length[r0 + j] : 0;
    }
    const long per_row = GW_MAX_BLOCKS / nr;  // >= 32
    const long need = (row_len + GW_BLOCK * 4 - 1) / (GW_BLOCK * 4);
    const dim3 grid((unsigned)(need < per_row ? need : per_row), (unsigned)nr);
    float* o = out + (int64_t)r0 * out_stride;
    if (vec_out)
      hipLaunchKernelGGL((k_gather_windows<true>), grid, dim3(GW_BLOCK), 0, s, arena, g, (long)row_len, o,
                         (long)out_stride);
    else
      hipLaunchKernelGGL((k_gather_windows<false>), grid, dim3(GW_BLOCK), 0, s, arena, g, (long)row_len, o,
                         (long)out_stride);
    const int rc = tw_check_launch(name);
    if (rc) return rc;
  }
  return 0;
}
