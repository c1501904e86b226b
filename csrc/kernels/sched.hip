// The learning-rate schedule's device side (dg_lr_sched: module _dgsched, sched_bindings.cpp,
// loaded only for lr_schedule != none).  deep_go_amd/train/optim.py LRSchedule / lr_factor is the
// definition.  The rate is a device double that the optimizer kernels and grad_update read
// inside the captured step graph, so the schedule is a launch on the step's stream too: the last
// of optimizer_step, behind the launch that decays lr.  It overwrites that decay with
//
//   base = base * (1 - rate_decay);  s = s + 1                       (advance = 1 only)
//   w    = min(1, (s + 1) / W)  for W > 0, else 1
//   u    = clamp((s - W) / (T - W), 0, 1)
//   d    = 1 | 1 - (1 - m) u | m + (1 - m) 0.5 (1 + cos(pi u)) | max(m, g ^ floor(max(s - W, 0) / E))
//          (constant | linear | cosine | step; linear and cosine: exactly m for s >= T)
//   *lr  = base * (w * d)
//
// all in double, every operation rounded once (no contraction).  s counts every step, applied
// or skipped, as the decay does: the launch takes no gate.  base and s live in a 16-byte device
// record.  One wave, one lane: the same lane reads and writes the record, so no thread reads
// what another thread of the launch writes.  No atomics, allocations or host syncs.
#include <cmath>

#include "dg_api.h"
#include "dg_common.h"

namespace {

struct SchedRecord {
  double base;
  long long s;
};
static_assert(sizeof(SchedRecord) == 16, "the record's layout is part of the interface");

enum : int { K_CONSTANT = 0, K_LINEAR = 1, K_COSINE = 2, K_STEP = 3 };

constexpr double PI = 3.141592653589793;     // (the double next to pi: Python's math.pi)

// g^k for an integer k >= 0 by squaring in double-double arithmetic (the product's error from
// an fma, one renormalisation per product), rounded once at the end: about 100 bits carried
// through at most 63 squarings, so the result is the correctly rounded power short of a near
// tie, as the host's pow is.  The device library's pow is not: it returned 0.5^4 one ulp low,
// and a plateau of lr_schedule=step is rate * g^k exactly.
struct DD {
  double h, l;
};

__device__ DD dd_mul(DD a, DD b) {
#pragma clang fp contract(off)
  const double p = a.h * b.h;
  double e = fma(a.h, b.h, -p);
  e = e + (a.h * b.l + a.l * b.h);
  const double h = p + e;
  return {h, e - (h - p)};
}

__device__ double powi(double g, long long k) {
  DD r{1.0, 0.0}, b{g, 0.0};
  for (; k > 0; k >>= 1) {
    if (k & 1) r = dd_mul(r, b);
    b = dd_mul(b, b);
  }
  return r.h;
}

__device__ double sched_factor(int kind, long long s, long long W, long long T, double m,
                               long long E, double g) {
#pragma clang fp contract(off)
  double w = 1.0;
  if (W > 0) {
    w = ((double)s + 1.0) / (double)W;
    w = w < 1.0 ? w : 1.0;
  }
  double d = 1.0;
  if (kind == K_LINEAR || kind == K_COSINE) {
    if (s >= T) {
      d = m;                                   // past the horizon the factor stays at the floor
    } else {
      double u = (double)(s - W) / (double)(T - W);
      u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
      if (kind == K_LINEAR) {
        d = 1.0 - (1.0 - m) * u;
      } else {
        // (u == 0 through the warm-up: the cosine is then 1 whatever the library's error)
        const double c = u == 0.0 ? 1.0 : cos(PI * u);
        d = m + (1.0 - m) * (0.5 * (1.0 + c));
      }
    }
  } else if (kind == K_STEP) {
    const long long k = (s > W ? s - W : 0) / E;
    const double p = powi(g, k);
    d = m > p ? m : p;
  }
  return w * d;
}

__global__ void __launch_bounds__(64)
lr_sched_tick(SchedRecord* __restrict__ rec, double* __restrict__ lr, int kind, long long W,
              long long T, double m, long long E, double g, double rate_decay, int advance) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  double base = rec->base;
  long long s = rec->s;
  if (advance) {
    base = base * (1.0 - rate_decay);
    s = s + 1;
    rec->base = base;
    rec->s = s;
  }
  *lr = base * sched_factor(kind, s, W, T, m, E, g);
}

// every refusal that config.override makes, and the pointers (written so that a NaN is refused
// too)
bool args_ok(const void* rec, const void* lr, int kind, long long W, long long T, double m,
             long long E, double g, double rate_decay, int advance) {
  if (!rec || !lr || (((uintptr_t)rec | (uintptr_t)lr) & 7)) return false;
  if (kind < K_CONSTANT || kind > K_STEP || (advance != 0 && advance != 1)) return false;
  if (W < 0 || T < 0 || E < 0) return false;
  if (!(m >= 0.0 && m <= 1.0) || !(g > 0.0 && g <= 1.0) || !std::isfinite(rate_decay))
    return false;
  if ((kind == K_LINEAR || kind == K_COSINE) && !(T > W)) return false;
  if (kind == K_STEP && !(E > 0)) return false;
  return true;
}

}  // namespace

extern "C" {

hipError_t dg_lr_sched(void* rec, double* lr, int kind, long long W, long long T, double m,
                       long long E, double g, double rate_decay, int advance, hipStream_t s) {
  // every refusal comes before any GPU work
  if (!args_ok(rec, lr, kind, W, T, m, E, g, rate_decay, advance)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lr_sched_tick, dim3(1), dim3(64), 0, s, (SchedRecord*)rec, lr, kind, W, T, m,
                     E, g, rate_decay, advance);
  return hipGetLastError();
}

}  // extern "C"
