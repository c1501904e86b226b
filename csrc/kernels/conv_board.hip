// Board-tiled implicit-GEMM convolution (forward and dgrad) for 3x3 / 1x1 layers with a
// multiple-of-64 input channel count — the hot path of every hidden layer.
//
// One workgroup (8 waves, 512 threads) computes a 128-output-channel x 1-board tile:
//   D[co][p] = sum_{chunk, tap, c} W[co][tap][chunk*64 + c] * X[b][p + off(tap)][chunk*64 + c]
// The board's whole zero-bordered frame (441 pixels for pad 1) for one 64-channel chunk is
// staged into LDS with global_load_lds_dwordx4 (double-buffered across chunks, the next
// chunk's DMA spread over the current chunk's tap steps), and every one of the 9 taps
// reads its B fragments from that halo image at a constant row offset — the input is
// fetched from L2 once per chunk instead of once per tap (the per-tap im2col tile of
// conv_nt_kernel).  Weight tiles [128 co][64 k] stream per tap step (double-buffered).
//
// LDS rows are 128 B (64 bf16); the 16-B slot of k-group g in row r is g ^ (r & 7),
// applied on the DMA source address (destinations of LDS-DMA are lane-linear), which
// keeps the ds_read_b128 fragment reads bank-conflict-free.
//
// Wave layout: WM x WN = 8 waves; each wave owns MF x NF 16x16 fragments
// (v_mfma_f32_16x16x32_bf16): BM = 128 -> 2 x 4 waves, 4 x 6 fragments; BM = 64 -> 1 x 8
// waves, 4 x 3 fragments.  N covers 384 >= 361 pixel columns (6% padding).
#include "dg_api.h"
#include "dg_common.h"

using namespace dg;

namespace {

constexpr int NCOL = 384;

struct BoardArgs {
  const bf16_t* A;     // [Mpad][KP] weights, k = tap*x_C + ci
  const char* X;       // input frame [B][F][F][x_C]
  char* Y;             // output frame [B][Fy][Fy][M]
  const float* bias;   // [M]       (EPI_FWD)
  const float* posb;   // [361][M]  (EPI_FWD)
  const char* aux;     // [B][Fa][Fa][M] mask frame (EPI_DGRAD)
  int KP;
  int M;
  int x_pad, x_C;
  int y_pad;
  int aux_pad;
  const bf16_t* pbias;  // [361][M] bf16 bias + pos_bias (EPI_FWD; replaces bias/posb if set)
  uint8_t* mask;        // [B][361][M/8] ReLU bitmask: written by EPI_FWD, read by EPI_DGRAD
                        // (replaces the aux frame) — 1 bit instead of a bf16 per element
  int ablate;  // diagnostics (tools/kbench.py): 1 no MFMA, 2 no LDS reads, 4 no DMA,
              // 8 no epilogue, 16 no per-step barrier (timing only)
};

// HB = halo buffers: 2 double-buffers the per-chunk halo (one workgroup per CU, BM = 128);
// 1 keeps a single halo image (73 KB of LDS at BM = 64), so TWO workgroups share a CU and
// one's prologue / chunk-switch / epilogue runs under the other's MFMAs.
template <int KW, int WM, int EPI, int HB>
__global__ void __launch_bounds__(512, (WM == 1 ? 2 : 1))
conv_board_kernel(BoardArgs a) {
  constexpr int WN = 8 / WM;
  constexpr int MF = 4;                   // 64 rows per wave
  constexpr int NF = NCOL / (16 * WN);    // 6 (WN=4) or 3 (WN=8)
  constexpr int BM = 64 * WM;
  constexpr int R = (KW - 1) / 2;
  constexpr int T = KW * KW;
  constexpr int A_BYTES = BM * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int b = blockIdx.x;
  const int m_tile = blockIdx.y * BM;
  const int F = BOARD + 2 * a.x_pad;
  const int FF = F * F;
  const int HROWS = (FF + 63) / 64 * 64;  // halo rows padded to whole 8-wave DMA rounds
  const int H_BYTES = HROWS * 128;
  char* sA0 = smem;
  char* sH0 = smem + 2 * A_BYTES;

  const int nchunk = a.x_C / 64;
  const int nsteps = nchunk * T;
  const char* Xb = a.X + (size_t)b * FF * a.x_C * 2;

  // ---- DMA issue helpers ----
  const int g_src = (lane & 7) ^ (lane >> 3);  // source swizzle: row&7 == lane>>3
  const bool no_mfma = a.ablate & 1, no_lds = a.ablate & 2, no_dma = a.ablate & 4;
  auto stage_A = [&](int buf, int step) {
    if (no_dma) return;
    const int c = step / T, t = step - (step / T) * T;
    const int kcol = t * a.x_C + c * 64;  // first k of this step
    char* dst = sA0 + buf * A_BYTES;
    constexpr int INSTR = BM / 8 / 8;     // 1 KiB instrs per wave: BM rows / 8 rows / 8 waves
#pragma unroll
    for (int i = 0; i < INSTR; ++i) {
      const int r = (wave * INSTR + i) * 8 + (lane >> 3);
      glds16((const char*)a.A + ((size_t)(m_tile + r) * a.KP + kcol + g_src * 8) * 2,
             (LDS_AS void*)(dst + (wave * INSTR + i) * 1024));
    }
  };
  // halo instruction j (0 .. HROWS/8-1) of chunk c: rows 8j .. 8j+7
  auto stage_H_instr = [&](int buf, int c, int j) {
    if (no_dma) return;
    int r = j * 8 + (lane >> 3);
    const int rs = r < FF ? r : FF - 1;
    glds16(Xb + ((size_t)rs * a.x_C + c * 64 + g_src * 8) * 2,
           (LDS_AS void*)(sH0 + buf * H_BYTES + j * 1024));
  };
  const int h_instr_total = HROWS / 8;          // e.g. 56
  const int h_per_wave = h_instr_total / 8;     // e.g. 7

  // ---- per-lane B-fragment row bases (frame pixel of each column) ----
  const int lr = lane & 15;
  const int lq = lane >> 4;
  int fp[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    int p = wn * NF * 16 + j * 16 + lr;
    if (p >= NPTS) p = 0;
    const int h = p / BOARD, w = p - (p / BOARD) * BOARD;
    fp[j] = (h + a.x_pad) * F + (w + a.x_pad);
  }

  f32x4 acc[MF][NF];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: halo of chunk 0 + weights of step 0 ----
  for (int j = wave; j < h_instr_total; j += 8) stage_H_instr(0, 0, j);
  stage_A(0, 0);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const int c = s / T, t = s - (s / T) * T;
    if (s + 1 < nsteps) stage_A((s + 1) & 1, s + 1);
    // spread the next chunk's halo DMA over this chunk's tap steps: wave-local instruction
    // k (0 .. h_per_wave-1) at step t = k; whatever is left (and the 8-wave remainder) at
    // the chunk's last step, so the whole halo has landed by the barrier ending the chunk.
    if (HB == 2 && c + 1 < nchunk) {
      if (t < T - 1) {
        if (t < h_per_wave) stage_H_instr((c + 1) & 1, c + 1, wave * h_per_wave + t);
      } else {
        for (int k = T - 1; k < h_per_wave; ++k)
          stage_H_instr((c + 1) & 1, c + 1, wave * h_per_wave + k);
        for (int j = 8 * h_per_wave + wave; j < h_instr_total; j += 8)
          stage_H_instr((c + 1) & 1, c + 1, j);
      }
    }
    const char* sA = sA0 + (s & 1) * A_BYTES;
    const char* sH = sH0 + (HB == 2 ? (c & 1) * H_BYTES : 0);
    const int toff = (t / KW - R) * F + (t % KW - R);
    // all 20 fragment reads of the step are issued before the first MFMA (distinct
    // registers), so the k-half 0 MFMAs only wait for their own operands and the k-half 1
    // reads complete underneath them.
    bf16x8 af[2][MF], bfr[2][NF];
    if (no_lds) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < MF; ++i) af[kk][i] = bf16x8{};
#pragma unroll
        for (int j = 0; j < NF; ++j) bfr[kk][j] = bf16x8{};
      }
    } else
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int g = kk * 4 + lq;
#pragma unroll
      for (int i = 0; i < MF; ++i)
        af[kk][i] = lds_read_b128(
            (const LDS_AS char*)(sA + (wm * 64 + i * 16 + lr) * 128 + ((g ^ (lane & 7)) * 16)));
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int row = fp[j] + toff;
        bfr[kk][j] = lds_read_b128((const LDS_AS char*)(sH + row * 128 + ((g ^ (row & 7)) * 16)));
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // keep every read above the MFMA block
    if (no_mfma) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < MF; ++i) asm volatile("" ::"v"(af[kk][i]));
#pragma unroll
        for (int j = 0; j < NF; ++j) asm volatile("" ::"v"(bfr[kk][j]));
      }
    } else
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = mfma16(af[kk][i], bfr[kk][j], acc[i][j]);
    // keep the DMA wait + barrier BELOW the MFMAs so they hide the next tile's DMA latency
    __builtin_amdgcn_sched_barrier(0);
    if (!(a.ablate & 16)) __syncthreads();
    if (HB == 1 && t == T - 1 && c + 1 < nchunk) {
      // single halo image: every wave is past its reads of chunk c (barrier above)
      for (int j = wave; j < h_instr_total; j += 8) stage_H_instr(0, c + 1, j);
      __syncthreads();
    }
  }

  if (a.ablate & 8) {
    float keep = 0.f;
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) keep += acc[i][j][0];
    if (keep == 1234.5f) a.Y[0] = 1;  // keep the MFMAs alive
    return;
  }
  // ---- epilogue: fragments -> LDS tile [361][BM] bf16 -> coalesced 16-byte row stores ----
  // (8-byte per-fragment stores cost ~12 us of a 40 us kernel: store-issue bound.)
  // Tile rows are BM*2 bytes; the 16-byte chunk c of row p lives at chunk c ^ (p & CMASK)
  // so the 16 pixel-rows written by one ds_write_b64 wave-instruction hit distinct banks.
  constexpr int NCH = BM / 8;        // 16-byte chunks per tile row
  constexpr int CMASK = NCH - 1;
  constexpr int ROWB = BM * 2;
  f32x4 bb[MF];
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    const int co = m_tile + wm * 64 + i * 16 + lq * 4;
    if constexpr (EPI == EPI_FWD)
      bb[i] = a.pbias ? f32x4{0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(a.bias + (co < a.M ? co : 0));
  }
  f32x4 pb[NF][MF];
  if constexpr (EPI == EPI_FWD) {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      int p = wn * NF * 16 + j * 16 + lr;
      p = p < NPTS ? p : 0;
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        const int co = m_tile + wm * 64 + i * 16 + lq * 4;
        const int cc = co < a.M ? co : 0;
        if (a.pbias) {  // combined bf16 table: 8 B per 4 channels instead of 16 B + bias
          const uint2 u = *(const uint2*)(a.pbias + p * a.M + cc);
          pb[j][i] = f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u),
                           __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xFFFF0000u)};
        } else {
          pb[j][i] = *(const f32x4*)(a.posb + p * a.M + cc);
        }
      }
    }
  }
  char* sT = smem;  // reuses the (drained) staging buffers
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int p = wn * NF * 16 + j * 16 + lr;
    if (p >= NPTS) continue;
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const int col = wm * 64 + i * 16 + lq * 4;  // channel within the tile
      f32x4 v = acc[i][j];
      if constexpr (EPI == EPI_FWD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r] + bb[i][r] + pb[j][i][r], 0.f);
      }
      uint2 o;
      o.x = pack_bf16x2(v[0], v[1]);
      o.y = pack_bf16x2(v[2], v[3]);
      const int chunk = (col >> 3) ^ (p & CMASK);
      *(uint2*)(sT + p * ROWB + chunk * 16 + (col & 4) * 2) = o;
    }
  }
  __syncthreads();
  const int Fy = BOARD + 2 * a.y_pad;
  const int Fa = BOARD + 2 * a.aux_pad;
  char* Yb = a.Y + (size_t)b * Fy * Fy * a.M * 2;
  const char* Ab = a.aux + (size_t)b * Fa * Fa * a.M * 2;
  for (int idx = tid; idx < NPTS * NCH; idx += 512) {
    const int p = idx / NCH, c = idx - (idx / NCH) * NCH;
    const int co = m_tile + c * 8;
    if (co >= a.M) continue;
    const int h = p / BOARD, w = p - (p / BOARD) * BOARD;
    uint4 v = *(const uint4*)(sT + p * ROWB + ((c ^ (p & CMASK)) * 16));
    const size_t mbyte = ((size_t)b * NPTS + p) * (a.M >> 3) + (co >> 3);
    if constexpr (EPI == EPI_FWD) {
      if (a.mask) {  // post-ReLU: bit = value != 0 (== value > 0)
        auto nz = [](uint32_t u) { return ((u & 0xFFFFu) ? 1u : 0u) | ((u >> 16) ? 2u : 0u); };
        a.mask[mbyte] = (uint8_t)(nz(v.x) | (nz(v.y) << 2) | (nz(v.z) << 4) | (nz(v.w) << 6));
      }
    }
    if constexpr (EPI == EPI_DGRAD) {
      if (a.mask) {
        const uint32_t mb = a.mask[mbyte];
        auto keep = [](uint32_t val, uint32_t bits) {
          return val & (((bits & 1u) ? 0xFFFFu : 0u) | ((bits & 2u) ? 0xFFFF0000u : 0u));
        };
        v.x = keep(v.x, mb);
        v.y = keep(v.y, mb >> 2);
        v.z = keep(v.z, mb >> 4);
        v.w = keep(v.w, mb >> 6);
        *(uint4*)(Yb + (size_t)(((h + a.y_pad) * Fy + (w + a.y_pad)) * a.M + co) * 2) = v;
        continue;
      }
      const uint4 m = *(const uint4*)(Ab + (size_t)(((h + a.aux_pad) * Fa + (w + a.aux_pad)) * a.M + co) * 2);
      // keep the gradient where the activation is > 0 (bf16: sign clear and non-zero)
      auto gate = [](uint32_t val, uint32_t msk) {
        uint32_t keep = 0;
        if ((msk & 0xFFFFu) != 0 && !(msk & 0x8000u)) keep |= 0xFFFFu;
        if ((msk >> 16) != 0 && !(msk & 0x80000000u)) keep |= 0xFFFF0000u;
        return val & keep;
      };
      v.x = gate(v.x, m.x);
      v.y = gate(v.y, m.y);
      v.z = gate(v.z, m.z);
      v.w = gate(v.w, m.w);
    }
    *(uint4*)(Yb + (size_t)(((h + a.y_pad) * Fy + (w + a.y_pad)) * a.M + co) * 2) = v;
  }
}

template <typename K>
void allow_lds(K kernel, size_t bytes) {
  static size_t done = 0;
  if (bytes > done) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
    done = bytes;
  }
}

template <int KW, int WM, int EPI, int HB>
hipError_t launch_hb(const BoardArgs& a, int B, int Mpad, hipStream_t s) {
  const int F = 19 + 2 * a.x_pad;
  const int hrows = (F * F + 63) / 64 * 64;
  size_t lds = 2 * (size_t)(64 * WM * 128) + HB * (size_t)hrows * 128;
  const size_t epi = (size_t)NPTS * 64 * WM * 2;  // epilogue tile reuses the staging area
  if (epi > lds) lds = epi;
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  allow_lds(conv_board_kernel<KW, WM, EPI, HB>, lds);
  hipLaunchKernelGGL((conv_board_kernel<KW, WM, EPI, HB>), dim3(B, Mpad / (64 * WM)), dim3(512),
                     lds, s, a);
  return hipGetLastError();
}

// HB = 1 (single halo image) at BM = 64 (two workgroups per CU) and whenever the input has a
// single 64-channel chunk (nothing to double-buffer); else HB = 2.
template <int KW, int WM, int EPI>
hipError_t launch(const BoardArgs& a, int B, int Mpad, hipStream_t s) {
  if (WM == 1 || a.x_C == 64) return launch_hb<KW, WM, EPI, 1>(a, B, Mpad, s);
  return launch_hb<KW, WM, EPI, 2>(a, B, Mpad, s);
}

template <int KW, int WM>
hipError_t dispatch_epi(int epi, const BoardArgs& a, int B, int Mpad, hipStream_t s) {
  switch (epi) {
    case EPI_FWD: return launch<KW, WM, EPI_FWD>(a, B, Mpad, s);
    case EPI_DGRAD: return launch<KW, WM, EPI_DGRAD>(a, B, Mpad, s);
    default: return launch<KW, WM, EPI_LINEAR>(a, B, Mpad, s);
  }
}

}  // namespace

static int g_board_ablate = 0;
extern "C" void dg_conv_board_set_ablate(int mode) { g_board_ablate = mode; }

extern "C" hipError_t dg_conv_board_ex(int epi, int kw, int bm, const void* A, int KP, int M,
                                       int Mpad, const void* X, int x_pad, int x_C, int B,
                                       void* Y, int y_pad, const float* bias, const float* posb,
                                       const void* pbias, const void* aux, int aux_pad,
                                       void* mask, hipStream_t stream) {
  if (x_C % 64 != 0 || M % 8 != 0 || (bm != 64 && bm != 128) || Mpad % bm != 0 || B <= 0)
    return hipErrorInvalidValue;
  if (KP < kw * kw * x_C || x_pad < (kw - 1) / 2) return hipErrorInvalidValue;
  if (epi == EPI_DGRAD && !aux && !mask) return hipErrorInvalidValue;
  BoardArgs a{(const bf16_t*)A, (const char*)X, (char*)Y, bias, posb, (const char*)aux, KP, M,
              x_pad, x_C, y_pad, aux_pad, (const bf16_t*)pbias, (uint8_t*)mask,
              g_board_ablate};
  const int wm = bm / 64;
  switch (kw) {
    case 1: return wm == 2 ? dispatch_epi<1, 2>(epi, a, B, Mpad, stream)
                           : dispatch_epi<1, 1>(epi, a, B, Mpad, stream);
    case 3: return wm == 2 ? dispatch_epi<3, 2>(epi, a, B, Mpad, stream)
                           : dispatch_epi<3, 1>(epi, a, B, Mpad, stream);
    case 5: return wm == 2 ? dispatch_epi<5, 2>(epi, a, B, Mpad, stream)
                           : dispatch_epi<5, 1>(epi, a, B, Mpad, stream);
    default: return hipErrorInvalidValue;
  }
}

extern "C" hipError_t dg_conv_board(int epi, int kw, int bm, const void* A, int KP, int M,
                                    int Mpad, const void* X, int x_pad, int x_C, int B, void* Y,
                                    int y_pad, const float* bias, const float* posb,
                                    const void* aux, int aux_pad, hipStream_t stream) {
  return dg_conv_board_ex(epi, kw, bm, A, KP, M, Mpad, X, x_pad, x_C, B, Y, y_pad, bias, posb,
                          nullptr, aux, aux_pad, nullptr, stream);
}
