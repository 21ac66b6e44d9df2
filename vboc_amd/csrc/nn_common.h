// Device helpers shared by the two NN trainers (fit.hip: the VBOC regressor, cls.hip: the HJR / AL classifier): the
// exact-f32 MFMA wrapper and its fragment-packed storage, the Philox minibatch sampler (random.sample's set method)
// and torch.optim.Adam's single-tensor update.  Each trainer is its own translation unit and includes this once;
// the sampler is templated on the trainer's argument record (fields st->seed, st->draws, n, n_new, Bt).
#ifndef VBOC_NN_COMMON_H
#define VBOC_NN_COMMON_H

#include <hip/hip_runtime.h>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int TBL = 8192;     // sampler hash slots (>= 2 x the largest sample of one range)
constexpr int MAXK = 4096;    // largest sample of one range
constexpr int ROUNDS = 128;   // rejection rounds before the (never expected) sequential completion

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Fragment-packed storage: the 16 x 16 block (RB, CB) of a matrix read as MFMA fragments "lane (lr, lq) takes
// [16 RB + lr][16 CB + 4 lq + s], s = 0..3" is 1 KB, lane-major: one wave-instruction loads it whole.
__host__ __device__ __forceinline__ size_t pk(int R, int C, int ncb) {
  return ((size_t)((R >> 4) * ncb + (C >> 4)) * 64 + (R & 15) + 16 * ((C & 15) >> 2)) * 4 + (C & 3);
}

__device__ __forceinline__ void philox(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0];
    const unsigned long long p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (unsigned)p1;
    c[3] = (unsigned)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ unsigned hslot(unsigned v) { return (v * 2654435761u) >> 19; }

// find-or-insert v (stored as v + 1) in the LDS table; returns its slot.  The table never holds more than
// MAXK = TBL / 2 values, so the probe ends.
__device__ __forceinline__ int tbl_insert(unsigned* keys, unsigned v) {
  int h = hslot(v);
  for (;;) {
    const unsigned old = atomicCAS(&keys[h], 0u, v + 1);
    if (old == 0u || old == v + 1) return h;
    h = (h + 1) & (TBL - 1);
  }
}

__device__ __forceinline__ bool tbl_has(const unsigned* keys, unsigned v) {
  int h = hslot(v);
  for (;;) {
    const unsigned k = keys[h];
    if (k == 0u) return false;
    if (k == v + 1) return true;
    h = (h + 1) & (TBL - 1);
  }
}

constexpr int SNT = 256;            // sampler threads (one workgroup of the forward kernel's shape)
constexpr int SL = MAXK / SNT;      // sample slots per thread

// 64 KB: the hash table, then the owners (reused for the sequential completion's values and, in the complement
// path, the marks and the compaction counts once the owners are no longer needed)
struct SampLds {
  unsigned keys[TBL];
  union {
    unsigned own[TBL];
    unsigned pendv[MAXK];
    struct {
      unsigned char mark[2 * MAXK];
      int cnt[SNT];
    } c;
  } u;
  int npend;
};

// kk <= n / 2 distinct values of [0, n); slot p < kk (thread p % SNT, register p / SNT) gets vals[p / SNT].
// Round r: every pending slot draws, inserts, and claims its value with key (r << 12 | p); the smallest key
// (earliest round, then lowest slot) owns the value and the other claimants draw again - the set of
// random.sample's "draw, redraw while already selected" loop.  With at most half of [0, n) taken a slot is
// pending after ROUNDS rounds with probability < 2^-128; such slots then take the smallest free values.
__device__ __forceinline__ void sample_set(SampLds& L, unsigned n, int kk, unsigned long long step,
                                           unsigned long long seed, unsigned range, unsigned (&vals)[SL]) {
  const int tid = threadIdx.x;
  for (int i = tid; i < TBL; i += SNT) {
    L.keys[i] = 0u;
    L.u.own[i] = 0xFFFFFFFFu;
  }
  if (tid == 0) L.npend = 0;
  __syncthreads();
  const unsigned thr = (0u - n) % n;
  unsigned pend = 0u;       // bit u: slot tid + SNT u still needs a value
  int slot[SL];
#pragma unroll
  for (int u = 0; u < SL; ++u) {
    if (tid + SNT * u < kk) pend |= 1u << u;
    vals[u] = 0u;
    slot[u] = 0;
  }
  int any = 1;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32) ^ (0x2545F491u + range);
  for (unsigned r = 0; r < ROUNDS && any; ++r) {
    // one Philox block per four slots and round (Lemire: a word below thr is rejected and the slot simply
    // stays pending)
    unsigned drew = 0u;
#pragma unroll
    for (int q = 0; q < SL / 4; ++q) {
      if ((pend >> (4 * q)) & 15u) {
        unsigned c[4] = {(unsigned)step, (unsigned)(step >> 32), (unsigned)(tid + SNT * q), r};
        philox(c, k0, k1);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int u = 4 * q + x;
          if ((pend >> u) & 1u) {
            const unsigned long long m = (unsigned long long)c[x] * n;
            if ((unsigned)m >= thr) {
              vals[u] = (unsigned)(m >> 32);
              slot[u] = tbl_insert(L.keys, vals[u]);
              atomicMin(&L.u.own[slot[u]], (r << 12) | (unsigned)(tid + SNT * u));
              drew |= 1u << u;
            }
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SL; ++u)
      if (((drew >> u) & 1u) && L.u.own[slot[u]] == ((r << 12) | (unsigned)(tid + SNT * u))) pend &= ~(1u << u);
    any = __syncthreads_or(pend != 0u);
  }
  if (!any) return;
  // sequential completion: each still-pending slot gets a ticket (kept in slot[]), thread 0 hands out the
  // smallest free values in ticket order
#pragma unroll
  for (int u = 0; u < SL; ++u)
    if ((pend >> u) & 1u) slot[u] = atomicAdd(&L.npend, 1);
  __syncthreads();
  if (tid == 0) {
    unsigned v = 0;
    for (int i = 0; i < L.npend; ++i) {
      while (tbl_has(L.keys, v)) ++v;
      tbl_insert(L.keys, v);
      L.u.pendv[i] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < SL; ++u)
    if ((pend >> u) & 1u) vals[u] = L.u.pendv[slot[u]];
  __syncthreads();
}

// indices of one range [lo, lo + n) into out[off, off + kk)
template <class A>
__device__ void sample_range(SampLds& L, const A& a, int* out, long long lo, unsigned n, int kk, int off,
                             unsigned long long step, unsigned range) {
  const int tid = threadIdx.x;
  const unsigned long long seed = a.st->seed;
  unsigned vals[SL];
  if (2 * (long long)kk <= (long long)n) {
    sample_set(L, n, kk, step, seed, range, vals);
#pragma unroll
    for (int u = 0; u < SL; ++u) {
      const int p = tid + SNT * u;
      if (p < kk) out[off + p] = (int)(lo + vals[u]);
    }
    __syncthreads();
    return;
  }
  // kk > n / 2 (then n <= 2 MAXK): draw the n - kk rows left out, keep the others in increasing order
  const int nc = (int)n - kk;
  if (nc > 0) sample_set(L, n, nc, step, seed, range, vals);
  __syncthreads();
  for (int i = tid; i < (int)n; i += SNT) L.u.c.mark[i] = 0;
  __syncthreads();
  if (nc > 0) {
#pragma unroll
    for (int u = 0; u < SL; ++u)
      if (tid + SNT * u < nc) L.u.c.mark[vals[u]] = 1;
  }
  __syncthreads();
  // block compaction: thread t owns values [VT t, VT t + VT)
  constexpr int VT = 2 * MAXK / SNT;
  int c = 0;
  for (int q = 0; q < VT; ++q) {
    const int v = VT * tid + q;
    if (v < (int)n && !L.u.c.mark[v]) ++c;
  }
  L.u.c.cnt[tid] = c;
  __syncthreads();
  for (int d = 1; d < SNT; d <<= 1) {
    const int add = tid >= d ? L.u.c.cnt[tid - d] : 0;
    __syncthreads();
    L.u.c.cnt[tid] += add;
    __syncthreads();
  }
  int pos = L.u.c.cnt[tid] - c;
  for (int q = 0; q < VT; ++q) {
    const int v = VT * tid + q;
    if (v < (int)n && !L.u.c.mark[v]) out[off + pos++] = (int)(lo + v);
  }
  __syncthreads();
}

// one minibatch into `out`: draw number st->draws of the sampler's stream (then st->draws + 1)
template <class A>
__device__ __forceinline__ void sample_minibatch(SampLds& L, const A& a, int* out) {
  auto* st = a.st;
  const unsigned long long step = st->draws;
  __syncthreads();
  if (a.n_new == 0) {
    sample_range(L, a, out, 0, (unsigned)a.n, a.Bt, 0, step, 0u);
  } else {
    const long long n_old = a.n - a.n_new;
    sample_range(L, a, out, 0, (unsigned)n_old, a.Bt / 2, 0, step, 1u);
    sample_range(L, a, out, n_old, (unsigned)a.n_new, a.Bt / 2, a.Bt / 2, step, 2u);
  }
  if (threadIdx.x == 0) st->draws = step + 1;
}

// acc[u] += A[16 rows][HP] (LDS, row stride LD) x B' for the column tile 16 (w + 4u) .. +15, B [HP][HP] given
// fragment-packed (pk(j, k, HP / 16), row j = output column j).  MFMA step s of group t sums k = 16t + 4 lq + s.  Two register sets
// of B fragments alternate (group t + 1's loads are in flight while group t's MFMAs issue); no copies between
// them, so the compiler's waits stay one group behind the loads.
template <int NT, int LD>
__device__ __forceinline__ void mfma_group(const float* A, int t, int lr, int lq, const f4 (&bv)[NT],
                                           f4 (&acc)[NT]) {
  const f4 av = *(const f4*)&A[lr * LD + 16 * t + 4 * lq];
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    acc[u] = mfma(av.x, bv[u].x, acc[u]);
    acc[u] = mfma(av.y, bv[u].y, acc[u]);
    acc[u] = mfma(av.z, bv[u].z, acc[u]);
    acc[u] = mfma(av.w, bv[u].w, acc[u]);
  }
}

template <int HP, int NT, int LD>
__device__ __forceinline__ void gemm_rows(const float* A, const float* B, int w, int lane, int lr, int lq,
                                          f4 (&acc)[NT]) {
  constexpr int TG = HP / 16;   // even for every instantiation (HP a multiple of 64)
  const float* bp[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) bp[u] = B + ((size_t)(w + 4 * u) * TG * 64 + lane) * 4;
  f4 b0[NT], b1[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) b0[u] = *(const f4*)bp[u];
  static_assert(TG % 2 == 0, "column groups come in pairs");
  for (int t = 0; t < TG; t += 2) {
#pragma unroll
    for (int u = 0; u < NT; ++u) b1[u] = *(const f4*)(bp[u] + 256 * (t + 1));
    mfma_group<NT, LD>(A, t, lr, lq, b0, acc);
    if (t + 2 < TG) {
#pragma unroll
      for (int u = 0; u < NT; ++u) b0[u] = *(const f4*)(bp[u] + 256 * (t + 2));
    }
    mfma_group<NT, LD>(A, t + 1, lr, lq, b1, acc);
  }
}

// Adam (torch.optim.Adam, single-tensor path, betas (0.9, 0.999), eps 1e-8, no weight decay):
// exp_avg.lerp_(g, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2);
// p.addcdiv_(exp_avg, exp_avg_sq.sqrt() / sqrt(1 - b2^t) + eps, value=-lr / (1 - b1^t))
struct AdamC {
  float step, bc2s;
};
__device__ __forceinline__ void adam(float& p, float& m, float& v, float g, const AdamC& k) {
  m = m + 0.1f * (g - m);
  v = v * 0.999f + 0.001f * g * g;
  const float den = sqrtf(v) / k.bc2s + 1e-8f;
  p = p + k.step * (m / den);
}

}  // namespace

#endif
