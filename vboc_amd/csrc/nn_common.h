// Device helpers shared by the three NN libraries (fit.hip: the VBOC regressor, cls.hip: the HJR / AL classifier,
// pool.hip: the AL pool): the exact-f32 MFMA wrapper and its fragment-packed storage, the Philox minibatch sampler
// (random.sample's set method), torch.optim.Adam's single-tensor update, the trainers' 16-row forward pass
// (layer0_rows, gemm_rows, forward_rows), the output stage of every forward kernel of the three files (out_partials,
// out_sum) and the float64 ray arithmetic of the two RMSE marches (ray_step, ray_point, ray_norm).  Each library is its
// own translation unit with its own compile flags and includes this once; the sampler is templated on the trainer's
// argument record (fields st->seed, st->draws, n, n_new, Bt).
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

// Layer 0 of the trainers' 16-row forward pass: H1 = relu(x W0' + b0) into LDS at row stride LD, one hidden column
// per thread (k-ordered fma chain over the inputs).  xs holds the rows' inputs [16][NIN]; store(c, h) receives column
// c's 16 values (k_fwd_bwd packs them for dW1; the forward-only kernels' NoStore does nothing).  The caller's barriers
// stand before and after.
struct NoStore {
  __device__ __forceinline__ void operator()(int, const float (&)[16]) const {}
};
template <int NIN, int HP, int LD, class Store>
__device__ __forceinline__ void layer0_rows(const float* W0, const float* b0, const float* xs, float* H1,
                                            Store&& store) {
  for (int c = threadIdx.x; c < HP; c += 256) {
    float wc[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) wc[i] = W0[c * NIN + i];
    const float bc = b0[c];
    float h[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NIN; ++i) s = fmaf(xs[r * NIN + i], wc[i], s);
      h[r] = fmaxf(s + bc, 0.f);
      H1[r * LD + c] = h[r];
    }
    store(c, h);
  }
}

// The output stage after the hidden product, for RB blocks of 16 rows and NO outputs: acc[rb][u][g] holds
// A2[row 16 rb + 4 lq + g][col j = 16 (w + 4u) + lr].  acc becomes H2 = relu(A2 + b1) (the backward half reads it),
// each output's partial sum runs over the wave's columns in u order (one fma chain), then over the 16 lanes of a
// row by xor shuffles; lane lr == 0 writes red[w][row][o] (red is [4][16 RB][NO]).  b1 starts at Pb[ob1], W2
// ([NO][ldw]) at Pw[ow2]: the trainers keep both at constant offsets of one buffer, and given this way the offsets
// fold into the loads.  The caller puts a barrier between this and out_sum.
template <int NO, int RB, int NT>
__device__ __forceinline__ void out_partials(f4 (&acc)[RB][NT], const float* Pb, int ob1, const float* Pw, int ow2,
                                             int ldw, int w, int lr, int lq, float* red) {
  float op[RB][4][NO];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int o = 0; o < NO; ++o) op[rb][g][o] = 0.f;
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int j = 16 * (w + 4 * u) + lr;
    const float bj = Pb[ob1 + j];
    float wj[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) wj[o] = Pw[ow2 + o * ldw + j];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float h = fmaxf(acc[rb][u][g] + bj, 0.f);
        acc[rb][u][g] = h;
#pragma unroll
        for (int o = 0; o < NO; ++o) op[rb][g][o] = fmaf(h, wj[o], op[rb][g][o]);
      }
  }
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int d = 1; d < 16; d <<= 1)
#pragma unroll
        for (int o = 0; o < NO; ++o) op[rb][g][o] += __shfl_xor(op[rb][g][o], d);
    }
  if (lr == 0) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int o = 0; o < NO; ++o) red[((w * RB + rb) * 16 + 4 * lq + g) * NO + o] = op[rb][g][o];
  }
}

// output o of row r over the four waves, in wave order (the output bias is the caller's)
template <int NO, int RB>
__device__ __forceinline__ float out_sum(const float* red, int r, int o) {
  constexpr int W = 16 * RB * NO;
  return ((red[r * NO + o] + red[W + r * NO + o]) + red[2 * W + r * NO + o]) + red[3 * W + r * NO + o];
}

// The trainers' forward pass over 16 rows, called by all 256 threads: layer 0 into H1 (row stride HP + 4), a barrier,
// H2 = relu(H1 W1' + b1) on MFMA (wave w owns column tiles w + 4u; acc keeps H2 for the backward half) and the NO
// outputs' per-wave partials into red [4][16][NO].  Ly gives the offsets W0, B0, B1, W2 in the parameter buffer P.
// xs was written before a barrier of the caller's, and a barrier of the caller's stands between this and out_sum.
template <int NIN, int HP, int NO, class Ly, class Store = NoStore>
__device__ __forceinline__ void forward_rows(const float* P, const float* Wf, const float* xs, float* H1, float* red,
                                             f4 (&acc)[HP / 64], Store&& store = Store()) {
  constexpr int NT = HP / 64, LD = HP + 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  layer0_rows<NIN, HP, LD>(P + Ly::W0, P + Ly::B0, xs, H1, store);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NT; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
  gemm_rows<HP, NT, LD>(H1, Wf, w, lane, lr, lq, acc);
  out_partials<NO, 1, NT>(reinterpret_cast<f4(&)[1][NT]>(acc), P, Ly::B1, P, Ly::W2, HP, w, lr, lq, red);
}

// The float64 ray arithmetic of the two RMSE marches (HJR/triplependulum_hjr.py:150-176, AL/triplependulum_al.py:
// 204-227).
//
// `v0 - 1e-2 * X_test[i][3] / vel_norm`: (1e-2 * x) / vel_norm, subtracted for label 0 and added for label 1
__device__ __forceinline__ double ray_step(double v0, double vel_norm, int label) {
  return (label ? -1.0 : 1.0) * ((1e-2 * v0) / vel_norm);
}

// the velocity of point r + 1 past the base v: r + 1 sequential subtractions (the reference's own accumulation)
template <int NQ>
__device__ __forceinline__ void ray_point(double (&v)[NQ], const double (&c)[NQ], int r) {
  for (int k = 0; k <= r; ++k) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) v[i] = v[i] - c[i];
  }
}

// |v| (NQ >= 2); `sn` is the norm the stop test takes: |v[0 .. od)| where `partial` (then 1 <= od < NQ), else |v|
// itself.  The sum of squares starts from v0^2 + v1^2 and takes the later terms in index order.  FUSED = false (pool.hip,
// compiled without contraction) rounds every product and every sum, as NumPy does.  FUSED = true (cls.hip) is what
// contraction made of the same sum when k_boundary was written, fma(v_i, v_i, ...) onto a rounded v1^2, written out so
// that the recorded marches do not rest on the compiler choosing the same products again.
template <int NQ, bool FUSED>
__device__ __forceinline__ double ray_norm(const double (&v)[NQ], int od, bool partial, double& sn) {
  auto add_sq = [](double s, double x) { return FUSED ? fma(x, x, s) : s + x * x; };
  double q2 = add_sq(v[1] * v[1], v[0]);
  double p2 = od == 1 ? v[0] * v[0] : q2;
#pragma unroll
  for (int i = 2; i < NQ; ++i) {
    q2 = add_sq(q2, v[i]);
    if (i < od) p2 = add_sq(p2, v[i]);
  }
  const double vn = sqrt(q2);
  sn = partial ? sqrt(p2) : vn;
  return vn;
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
