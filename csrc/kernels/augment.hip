// Training-time symmetry augmentation: every board of a packed batch (data/batch.py) is moved,
// in place, by one of the eight board symmetries.  deep_go_amd/data/symmetry.py holds the
// definition: augment_symmetries (which symmetry each board gets) and augment_batch (the numpy
// oracle of the whole transform).  The launcher is built into its own small extension, _dgaug
// (aug_bindings.cpp).
//
// The symmetries T_s, s in 0..7, of a point p = 19 x + y are sym_fwd / sym_inv of dg_common.h,
// the ones the predictor's ensemble (policy.hip) uses.
//
// The symmetry of a board is a pure 32-bit integer hash of (seed, loader sequence number, board
// index): no generator state, so a resumed run draws what the uninterrupted one would have, and
// the CPU path repeats it bit for bit.
#include "dg_api.h"
#include "dg_common.h"

using namespace dg;

namespace {

constexpr int PLANES = 9;      // stored uint8 planes per position (data/features.py)
constexpr int AT = 256;        // threads per workgroup
constexpr int BOARD_BYTES = PLANES * NPTS;

// augment_symmetries of data/symmetry.py, one board (mix32: dg_common.h)
__host__ __device__ inline int hash_symmetry(unsigned long long seed, unsigned long long seq,
                                             unsigned long long board) {
  const uint32_t a = mix32(((uint32_t)seed ^ 0x9e3779b9u) + (uint32_t)(seed >> 32));
  const uint32_t b = mix32(mix32(a + (uint32_t)seq) ^ (uint32_t)(seq >> 32));
  return (int)(mix32(b + (uint32_t)board) >> 29);
}

// One workgroup per board i: s = sym[i] & 7 when sym is given, else the hash of (seed, seq,
// board0 + i).  The board's nine planes are staged in LDS; after the barrier every thread
// writes destination points p from the inverse points (dst[p] = src[T_s^-1(p)], the same as
// dst[T_s(p)] = src[p]), so a wave's stores are contiguous.  Thread 0 moves the label (values
// outside 0..360 stay) and records s.  A board with s = 0 is not written.  No workgroup touches
// another board's bytes, so the in-place update needs no second buffer.
__global__ void __launch_bounds__(AT)
augment_batch_kernel(uint8_t* __restrict__ planes, int* __restrict__ labels,
                     const uint8_t* __restrict__ sym, unsigned long long seed,
                     unsigned long long seq, unsigned long long board0,
                     uint8_t* __restrict__ sym_out) {
  __shared__ uint8_t s_board[BOARD_BYTES];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int s = sym ? (sym[i] & 7) : hash_symmetry(seed, seq, board0 + (unsigned long long)i);
  if (tid == 0 && sym_out) sym_out[i] = (uint8_t)s;
  if (s == 0) return;                      // (the whole workgroup: s is uniform)
  uint8_t* board = planes + (size_t)i * BOARD_BYTES;
  for (int k = tid; k < BOARD_BYTES; k += AT) s_board[k] = board[k];
  __syncthreads();
  for (int p = tid; p < NPTS; p += AT) {
    const int q = sym_inv(s, p);
#pragma unroll
    for (int c = 0; c < PLANES; ++c) board[c * NPTS + p] = s_board[c * NPTS + q];
  }
  if (tid == 0) {
    const int y = labels[i];
    if (y >= 0 && y < NPTS) labels[i] = sym_fwd(s, y);
  }
}

}  // namespace

extern "C" {

int dg_augment_symmetry(unsigned long long seed, unsigned long long seq,
                        unsigned long long board) {
  return hash_symmetry(seed, seq, board);
}

hipError_t dg_augment_batch(uint8_t* planes, int* labels, int B, const uint8_t* sym,
                            unsigned long long seed, unsigned long long seq,
                            unsigned long long board0, uint8_t* sym_out, hipStream_t stream) {
  if (B < 0) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!planes || !labels) return hipErrorInvalidValue;
  hipLaunchKernelGGL(augment_batch_kernel, dim3(B), dim3(AT), 0, stream, planes, labels, sym,
                     seed, seq, board0, sym_out);
  return hipGetLastError();
}

}  // extern "C"
