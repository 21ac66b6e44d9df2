// The VBOC loop's NN fit on the device: Adam/MSE training of NeuralNetDIR (Linear-ReLU-Linear-ReLU-Linear-ReLU)
// with the reference's minibatch sampling and stop rule, one step = four kernels, `poll` steps per HIP graph.
//
// Reference: VBOC/triplependulum_vboc.py:415-466 (first fit: random.sample(range(n), 4096), MSE, Adam(lr 1e-3),
// val = 0.95 val + 0.05 loss, `while val > 1e-3 and it < it_max`), :526-556 (refits: 2048 rows from the old
// rows + 2048 from the new ones), my_nn.py:20-34 (the model), the double / pendulum twins.  What PyTorch runs
// there as ~40 small kernels per step (plus a host sync on loss.item()) is here:
//
//   k_fwd_bwd   the step's gate (val > stop && it < it_max); one extra workgroup draws the NEXT step's
//               minibatch, a uniform k-subset of each row range (Philox draws with rejection of repeats:
//               random.sample's set method; k_sample draws a fit's first one); 16 minibatch rows per other
//               workgroup (gathered from the feature rows): H1 = relu(x W0' + b0),
//               H2 = relu(H1 W1' + b1) and
//               dH1 = (dH2 W1) * [H1 > 0] on v_mfma_f32_16x16x4_f32 (exact f32, as the f32 GEMMs of PyTorch),
//               the output layer, the MSE gradient, per-workgroup partial gradients of every small parameter
//   k_dw1       dW1 = dH2' H1 (split over minibatch rows), plus the EMA / counter update of the reference's loop
//   k_adam      the partial sums reduced in a fixed order, torch.optim.Adam's update (single-tensor path),
//               W1 rewritten as the packed MFMA fragments of the next step's two products
//
// Beside the step (VBOC/vboc.py:564-642): k_prune selects the global L1 pruning mask, k_adam holds masked entries at
// zero during the refit under it, k_eval is the forward-only pass behind the RMSE and the safety margin.  k_fwd_bwd
// and k_eval run one forward pass, nn_common.h's forward_rows (k_fwd_bwd also packs H1 for dW1).
//
// Every operand streamed from L2 / MALL (W1 twice, H1 and dH2 for dW1) is stored fragment-packed (pk()): a wave's
// B (or A) fragment of one 16 x 16 block is 1 KB contiguous, so each load instruction moves whole 256-B lines.
//
// Every reduction has a fixed order, so a HIP-graph replay equals the eager launch sequence bit for bit; a step
// whose gate is 0 changes nothing, so running up to `poll - 1` steps past the stop is exact.  Parameters are kept
// in padded buffers (hidden rounded up to a multiple of 64; padding rows / columns stay exactly zero).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/vboc_fit.h"
#include "nn_common.h"

namespace {

constexpr int R2 = 16;        // minibatch rows per k_fwd_bwd workgroup

struct State {
  double val, stop, beta;
  long long it, it_lim, step_t;
  unsigned long long draws, seed;
  int gate, err, pad0, pad1;
};

struct Args {
  float* P;                   // parameters: [W0 (HP x NIN) | b0 | b1 | w2 (HP each) | b2 (4) | W1 (HP x HP)]
  float* M;                   // Adam exp_avg, same layout
  float* V;                   // Adam exp_avg_sq
  const float* K;             // 0 / 1 pruning mask, same layout (padding 0); null when no mask is active
  float* Wf;                  // W1 packed as the forward product's B fragments: pk(j, k, HP / 16)
  float* Wb;                  // W1 packed as the backward product's B fragments: element W1[j][c] at pk(c, j, HP / 16)
  int* idx;                   // this step's minibatch row indices [Bt]
  int* idx_next;              // the next step's, drawn by the forward kernel's extra workgroup
  float* H1p;                 // H1 packed as dW1's B fragments: element H1[r][c] at pk(c, r, Bt / 16)
  float* dH2p;                // dH2 packed as dW1's A fragments: element dH2[r][j] at pk(j, r, Bt / 16)
  float* part;                // per-workgroup partials [Bt / R2][REC]
  float* dW1p;                // split partials of dW1 [S][HP][HP]
  State* st;
  const float* F;             // feature rows [n][ldF]: NIN inputs then the target
  long long n, n_new;
  int ldF, Bt, S;
  float lr;
};

template <int NIN, int HP>
struct Lay {
  static constexpr int W0 = 0, B0 = HP * NIN, B1 = B0 + HP, W2 = B1 + HP, B2 = W2 + HP, SMALL = B2 + 4;
  static constexpr int W1 = SMALL, TOTAL = W1 + HP * HP, REC = SMALL + 4, LOSS = SMALL;
};

// the first minibatch of a fit (and the test hook vboc_fit_sample), into a.idx
__global__ __launch_bounds__(SNT) void k_sample(Args a) {
  __shared__ SampLds L;
  sample_minibatch(L, a, a.idx);
}

template <int NIN, int HP>
__global__ __launch_bounds__(256) void k_fwd_bwd(Args a) {
  using Ly = Lay<NIN, HP>;
  constexpr int NT = HP / 64;          // 16-column tiles per wave
  constexpr int LD = HP + 4;
  struct FwdLds {
    float H1[R2 * LD];
    float G2[R2 * LD];
    float xs[R2 * NIN], ys[R2], dout[R2], sq[R2], red[4][R2];
  };
  __shared__ __attribute__((aligned(16))) union {
    FwdLds f;
    SampLds s;
  } U;
  float* H1 = U.f.H1;
  float* G2 = U.f.G2;
  float* xs = U.f.xs;
  float* ys = U.f.ys;
  float* dout = U.f.dout;
  float* sq = U.f.sq;
  float (*red)[R2] = U.f.red;
  // the step's gate (the reference's `while val > stop and it < it_max`), from the state the previous step left;
  // block 0 publishes it for this step's dW1 / Adam kernels and the host's poll
  const State* sc = a.st;
  const int gate = (sc->val > sc->stop) && (sc->it < sc->it_lim);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.st->gate = gate;
  if (!gate) return;
  // the last workgroup draws the next step's minibatch (it reads nothing this step writes)
  if ((int)blockIdx.x == a.Bt / R2) {
    sample_minibatch(U.s, a, a.idx_next);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int row0 = blockIdx.x * R2;
  const float* P = a.P;
  // the workgroup's minibatch rows, gathered from the feature matrix
  if (tid < R2 * (NIN + 1)) {
    const int r = tid / (NIN + 1), i = tid % (NIN + 1);
    const float v = a.F[(size_t)a.idx[row0 + r] * a.ldF + i];
    if (i < NIN) xs[r * NIN + i] = v;
    else ys[r] = v;
  }
  __syncthreads();

  // the forward pass; H1 is also written transposed for dW1.  acc[u][g] = H2[row 4 lq + g][col 16 (w + 4u) + lr]
  f4 acc[NT];
  auto pack_h1 = [&](int c, const float(&h)[R2]) {
    f4* dst = (f4*)(a.H1p + pk(c, row0, a.Bt / 16));
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[16 * q] = f4{h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]};
  };
  forward_rows<NIN, HP, 1, Ly>(P, a.Wf, xs, H1, &red[0][0], acc, pack_h1);
  __syncthreads();
  if (tid < R2) {
    const float s = out_sum<1, 1>(&red[0][0], tid, 0);
    const float o = fmaxf(s + P[Ly::B2], 0.f);
    const float e = o - ys[tid];
    dout[tid] = o > 0.f ? e * (2.f / (float)a.Bt) : 0.f;     // d mean((o - y)^2) / d o, through the last ReLU
    sq[tid] = e * e;
  }
  __syncthreads();

  float* part = a.part + (size_t)blockIdx.x * Ly::REC;
  float dr[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) dr[g] = dout[4 * lq + g];
  // dH2 = dout w2 [H2 > 0]; db1 and dw2 partials; dH2 to LDS and transposed to global
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int j = 16 * (w + 4 * u) + lr;
    const float wj = P[Ly::W2 + j];
    float gv[4], sb = 0.f, sw = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float h = acc[u][g];
      gv[g] = h > 0.f ? dr[g] * wj : 0.f;
      sb += gv[g];
      sw = fmaf(dr[g], h, sw);
      G2[(4 * lq + g) * LD + j] = gv[g];
    }
    *(f4*)(a.dH2p + pk(j, row0 + 4 * lq, a.Bt / 16)) = f4{gv[0], gv[1], gv[2], gv[3]};
    sb += __shfl_xor(sb, 16);
    sb += __shfl_xor(sb, 32);
    sw += __shfl_xor(sw, 16);
    sw += __shfl_xor(sw, 32);
    if (lq == 0) {
      part[Ly::B1 + j] = sb;
      part[Ly::W2 + j] = sw;
    }
  }
  if (tid == 0) {
    float s = 0.f, l = 0.f;
    for (int r = 0; r < R2; ++r) {
      s += dout[r];
      l += sq[r];
    }
    part[Ly::B2] = s;
    part[Ly::B2 + 1] = 0.f;
    part[Ly::B2 + 2] = 0.f;
    part[Ly::B2 + 3] = 0.f;
    part[Ly::LOSS] = l;
  }
  __syncthreads();

  // dH1 = dH2 W1 [H1 > 0] on MFMA (B operand W1[j][c], packed in Wb); db0 and dW0 partials
#pragma unroll
  for (int u = 0; u < NT; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
  gemm_rows<HP, NT, LD>(G2, a.Wb, w, lane, lr, lq, acc);
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int c = 16 * (w + 4 * u) + lr;
    float sb = 0.f, sw[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) sw[i] = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int r = 4 * lq + g;
      const float gg = H1[r * LD + c] > 0.f ? acc[u][g] : 0.f;
      sb += gg;
#pragma unroll
      for (int i = 0; i < NIN; ++i) sw[i] = fmaf(gg, xs[r * NIN + i], sw[i]);
    }
    sb += __shfl_xor(sb, 16);
    sb += __shfl_xor(sb, 32);
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      sw[i] += __shfl_xor(sw[i], 16);
      sw[i] += __shfl_xor(sw[i], 32);
    }
    if (lq == 0) {
      part[Ly::B0 + c] = sb;
#pragma unroll
      for (int i = 0; i < NIN; ++i) part[Ly::W0 + c * NIN + i] = sw[i];
    }
  }
}

// dW1 partials: workgroup = 64 x 64 output block x one of S row splits; wave = 32 x 32 (2 x 2 MFMA tiles).
// Block 0's first wave also applies the reference's loop update: val = beta val + (1 - beta) loss, it += 1.
template <int NIN, int HP>
__global__ __launch_bounds__(256) void k_dw1(Args a) {
  using Ly = Lay<NIN, HP>;
  State* st = a.st;
  if (!st->gate) return;
  constexpr int NB = HP / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int s = blockIdx.x / (NB * NB), b = blockIdx.x % (NB * NB);
  const int j0 = (b / NB) * 64 + (w >> 1) * 32, c0 = (b % NB) * 64 + (w & 1) * 32;
  const int KC = a.Bt / a.S, r0 = s * KC;
  f4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f4{0.f, 0.f, 0.f, 0.f};
  const int RG = a.Bt / 16;
  const float* A0 = a.dH2p + ((size_t)((j0 >> 4) * RG + (r0 >> 4)) * 64 + lane) * 4;
  const float* A1 = A0 + (size_t)RG * 256;
  const float* B0 = a.H1p + ((size_t)((c0 >> 4) * RG + (r0 >> 4)) * 64 + lane) * 4;
  const float* B1 = B0 + (size_t)RG * 256;
  auto group = [&](const f4 (&av)[2], const f4 (&bv)[2]) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        acc[x][y] = mfma(av[x].x, bv[y].x, acc[x][y]);
        acc[x][y] = mfma(av[x].y, bv[y].y, acc[x][y]);
        acc[x][y] = mfma(av[x].z, bv[y].z, acc[x][y]);
        acc[x][y] = mfma(av[x].w, bv[y].w, acc[x][y]);
      }
  };
  // ping-pong register sets, as gemm_rows
  f4 a0[2] = {*(const f4*)A0, *(const f4*)A1}, b0[2] = {*(const f4*)B0, *(const f4*)B1};
  f4 a1[2], b1[2];
  const int T = KC / 16;
  for (int t = 0; t < T; t += 2) {
    const int o1 = 256 * (t + 1), o2 = 256 * (t + 2);
    const bool odd = t + 1 < T;
    if (odd) {
      a1[0] = *(const f4*)(A0 + o1);
      a1[1] = *(const f4*)(A1 + o1);
      b1[0] = *(const f4*)(B0 + o1);
      b1[1] = *(const f4*)(B1 + o1);
    }
    group(a0, b0);
    if (t + 2 < T) {
      a0[0] = *(const f4*)(A0 + o2);
      a0[1] = *(const f4*)(A1 + o2);
      b0[0] = *(const f4*)(B0 + o2);
      b0[1] = *(const f4*)(B1 + o2);
    }
    if (odd) group(a1, b1);
  }
  float* out = a.dW1p + (size_t)s * HP * HP;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int g = 0; g < 4; ++g) out[(size_t)(j0 + 16 * x + 4 * lq + g) * HP + c0 + 16 * y + lr] = acc[x][y][g];
  if (blockIdx.x == 0 && w == 0) {
    const int nb = a.Bt / R2;
    float l = 0.f;
    for (int q = lane; q < nb; q += 64) l += a.part[(size_t)q * Ly::REC + Ly::LOSS];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o);
    if (lane == 0) {
      const float loss = l / (float)a.Bt;
      st->val = st->beta * st->val + (1.0 - st->beta) * (double)loss;
      st->it += 1;
      st->step_t += 1;
    }
  }
}

template <int NIN, int HP>
__global__ __launch_bounds__(256) void k_adam(Args a) {
  using Ly = Lay<NIN, HP>;
  __shared__ float tile[32][33];
  __shared__ float red[16][17];
  const State* st = a.st;
  if (!st->gate) return;
  const double t = (double)st->step_t;
  AdamC k;
  k.step = (float)(-(double)a.lr / (1.0 - pow(0.9, t)));
  k.bc2s = (float)sqrt(1.0 - pow(0.999, t));
  constexpr int NW1 = (HP / 32) * (HP / 32);
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < NW1) {
    const int tj = blockIdx.x / (HP / 32), tc = blockIdx.x % (HP / 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q, rj = e >> 5, rc = e & 31;
      const size_t o = (size_t)(tj * 32 + rj) * HP + tc * 32 + rc;
      float g = a.dW1p[o];
      for (int s = 1; s < a.S; ++s) g += a.dW1p[(size_t)s * HP * HP + o];
      // under a mask (prune.global_unstructured's reparametrisation, restated as zero-and-hold): the gradient
      // reaching a pruned entry is zero and the entry stays zero
      float mk = 1.f;
      if (a.K) {
        mk = a.K[Ly::W1 + o];
        g *= mk;
      }
      float p = a.P[Ly::W1 + o], m = a.M[Ly::W1 + o], v = a.V[Ly::W1 + o];
      adam(p, m, v, g, k);
      if (mk == 0.f) p = 0.f;
      a.P[Ly::W1 + o] = p;
      a.M[Ly::W1 + o] = m;
      a.V[Ly::W1 + o] = v;
      tile[rj][rc] = p;
    }
    __syncthreads();
    // the new W1 tile as the packed B fragments of both products: 4 blocks of 16 x 16 = 4 KB each, lane-major
    constexpr int TG = HP / 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q, bi = e >> 8, L = (e >> 2) & 63, sx = e & 3;
      const int b_r = bi >> 1, b_c = bi & 1, lr = L & 15, lq = L >> 4;
      // forward: rows j (output columns), k along the fragment
      a.Wf[(((size_t)(tj * 2 + b_r) * TG + tc * 2 + b_c) * 64 + L) * 4 + sx] = tile[16 * b_r + lr][16 * b_c + 4 * lq + sx];
      // backward: rows c, k = j along the fragment
      a.Wb[(((size_t)(tc * 2 + b_r) * TG + tj * 2 + b_c) * 64 + L) * 4 + sx] = tile[16 * b_c + 4 * lq + sx][16 * b_r + lr];
    }
    return;
  }
  // small parameters: 16 elements per workgroup, 16 partial-sum lanes each (fixed order)
  const int e = ((int)blockIdx.x - NW1) * 16 + (tid & 15), q = tid >> 4;
  const int nb = a.Bt / R2;
  float g = 0.f;
  if (e < Ly::SMALL)
    for (int wg = q; wg < nb; wg += 16) g += a.part[(size_t)wg * Ly::REC + e];
  red[q][tid & 15] = g;
  __syncthreads();
  if (q == 0 && e < Ly::SMALL) {
    float s = red[0][tid];
    for (int i = 1; i < 16; ++i) s += red[i][tid];
    float mk = 1.f;
    if (a.K) {
      mk = a.K[e];
      s *= mk;
    }
    float p = a.P[e], m = a.M[e], v = a.V[e];
    adam(p, m, v, s, k);
    if (mk == 0.f) p = 0.f;
    a.P[e] = p;
    a.M[e] = m;
    a.V[e] = v;
  }
}

// torch layouts <-> padded buffers
template <int NIN, int HP>
__global__ void k_pack(float* P, float* Wf, float* Wb, float* W0, float* b0, float* W1, float* b1, float* W2,
                       float* b2, int H, int unpack) {
  using Ly = Lay<NIN, HP>;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (long long)HP * HP) {
    const int j = (int)(i / HP), c = (int)(i % HP);
    if (unpack) {
      if (j < H && c < H) W1[j * H + c] = P[Ly::W1 + i];
    } else {
      const float v = (j < H && c < H) ? W1[j * H + c] : 0.f;
      P[Ly::W1 + i] = v;
      if (Wf) {
        Wf[pk(j, c, HP / 16)] = v;
        Wb[pk(c, j, HP / 16)] = v;
      }
    }
  }
  if (i < HP) {
    const int c = (int)i;
    if (unpack) {
      if (c < H) {
        for (int q = 0; q < NIN; ++q) W0[c * NIN + q] = P[Ly::W0 + c * NIN + q];
        b0[c] = P[Ly::B0 + c];
        b1[c] = P[Ly::B1 + c];
        W2[c] = P[Ly::W2 + c];
      }
      if (c == 0) b2[0] = P[Ly::B2];
    } else {
      for (int q = 0; q < NIN; ++q) P[Ly::W0 + c * NIN + q] = c < H ? W0[c * NIN + q] : 0.f;
      P[Ly::B0 + c] = c < H ? b0[c] : 0.f;
      P[Ly::B1 + c] = c < H ? b1[c] : 0.f;
      P[Ly::W2 + c] = c < H ? W2[c] : 0.f;
      if (c < 4) P[Ly::B2 + c] = c == 0 ? b2[0] : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// pruning (VBOC/vboc.py:564-625) and the forward-only evaluation (:555-559, :631-642)
// ------------------------------------------------------------------------------------------------
// The padded parameter layout with run-time sizes (Lay<NIN, HP> for the kernels that are no hot path).
struct LayR {
  int nin, hp, H, b0, b2, w1, total;
};

// a real (unpadded) entry of the layout
__device__ __forceinline__ bool lay_real(const LayR& L, int i) {
  if (i < L.b0) return i / L.nin < L.H;
  if (i < L.b2) return (i - L.b0) % L.hp < L.H;     // b0, b1, w2
  if (i < L.w1) return i == L.b2;
  const int o = i - L.w1;
  return o / L.hp < L.H && o % L.hp < L.H;
}

// the mask of an unpruned model: 1 on the real entries, 0 on the padding
__global__ void k_mask_ones(float* K, LayR L) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L.total) K[i] = lay_real(L, i) ? 1.f : 0.f;
}

// P = mask ? P : 0, and W1's packed fragments rewritten from it
__global__ void k_mask_apply(float* P, const float* K, float* Wf, float* Wb, LayR L) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.total) return;
  float v = P[i];
  if (K[i] == 0.f) {
    v = 0.f;
    P[i] = 0.f;
  }
  if (i >= L.w1) {
    const int o = i - L.w1, j = o / L.hp, c = o % L.hp;
    Wf[pk(j, c, L.hp / 16)] = v;
    Wb[pk(c, j, L.hp / 16)] = v;
  }
}

constexpr int PNT = 1024;           // k_prune's one workgroup

// L1Unstructured over all six tensors: the mask that drops the `nprune` real entries of smallest |p|.
// One workgroup.  The bit pattern of |p| is monotone in |p|, so the nprune-th smallest magnitude T is found by a
// radix select, most significant byte first: each pass histograms one byte of the keys that share the prefix found
// so far (per-wave LDS histograms, summed in wave order) and descends into the bin that holds the nprune-th key.
// Entries below T are pruned; of the entries equal to T the first `need` in buffer order (W0, b0, b1, W2, b2, W1,
// each row-major) are: every thread owns a contiguous index range, so an exclusive scan of the per-thread tie
// counts ranks the ties.  Integer counts only: the same parameters always give the same mask.
__global__ __launch_bounds__(PNT) void k_prune(const float* P, float* K, LayR L, long long nprune,
                                                long long* pruned) {
  __shared__ unsigned hist[PNT / 64][256];
  __shared__ unsigned tot[256];
  __shared__ unsigned cnt[PNT];
  __shared__ unsigned s_prefix, s_need, s_pruned;
  const int tid = threadIdx.x, wv = tid >> 6;
  unsigned prefix = 0u, need = (unsigned)nprune;      // the need-th smallest (from 1) of the keys under `prefix`
  if (tid == 0) s_pruned = 0u;
  for (int pass = 0; pass < 4 && nprune > 0; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < (PNT / 64) * 256; i += PNT) (&hist[0][0])[i] = 0u;
    __syncthreads();
    for (int i = tid; i < L.total; i += PNT) {
      if (!lay_real(L, i)) continue;
      const unsigned key = __float_as_uint(P[i]) & 0x7FFFFFFFu;
      if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[wv][(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 256) {
      unsigned s = 0u;
      for (int w = 0; w < PNT / 64; ++w) s += hist[w][tid];
      tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned cum = 0u;
      int b = 0;
      for (; b < 255; ++b) {
        if (cum + tot[b] >= need) break;
        cum += tot[b];
      }
      s_prefix = (prefix << 8) | (unsigned)b;
      s_need = need - cum;
    }
    __syncthreads();
    prefix = s_prefix;
    need = s_need;
    __syncthreads();
  }
  // prefix = the threshold key T, need = how many of the entries equal to T are pruned
  const int C = (L.total + PNT - 1) / PNT;
  const int lo = tid * C, hi = min(lo + C, L.total);
  unsigned c = 0u;
  if (nprune > 0)
    for (int i = lo; i < hi; ++i)
      if (lay_real(L, i) && (__float_as_uint(P[i]) & 0x7FFFFFFFu) == prefix) ++c;
  cnt[tid] = c;
  __syncthreads();
  for (int d = 1; d < PNT; d <<= 1) {
    const unsigned add = tid >= d ? cnt[tid - d] : 0u;
    __syncthreads();
    cnt[tid] += add;
    __syncthreads();
  }
  unsigned rank = cnt[tid] - c, np = 0u;
  for (int i = lo; i < hi; ++i) {
    float keep = 0.f;
    if (lay_real(L, i)) {
      const unsigned key = __float_as_uint(P[i]) & 0x7FFFFFFFu;
      const bool drop = nprune > 0 && (key < prefix || (key == prefix && rank++ < need));
      keep = drop ? 0.f : 1.f;
      np += drop;
    }
    K[i] = keep;
  }
  atomicAdd(&s_pruned, np);
  __syncthreads();
  if (tid == 0) *pruned = (long long)s_pruned;
}

constexpr int EVG = 2048;           // most workgroups (= partial records) of one evaluation

struct EvalArgs {
  const float* P;
  const float* Wf;
  const float* F;             // rows [n][ld]: NIN inputs (then the float32 target, read when y is null)
  const double* y;            // float64 targets [n], or null
  float* out;                 // model outputs [n], or null
  double* part;               // per-workgroup records [gridDim.x][3]: sum of squared errors, margin, rows above
  long long n;
  int ld, nblk;
};

// Forward only, through the training forward's own code (forward_rows: the W0 layer, gemm_rows on Wf, the output
// layer), 16 contiguous rows per workgroup and round; the last block's rows are loaded with clamped indices and masked
// on output.  Thread r < 16 keeps row r's running sums over the workgroup's blocks (in block order), thread 0 adds the
// 16 in lane order: a fixed order throughout, no floating-point atomics.
template <int NIN, int HP>
__global__ __launch_bounds__(256) void k_eval(EvalArgs e) {
  using Ly = Lay<NIN, HP>;
  constexpr int NT = HP / 64;
  constexpr int LD = HP + 4;
  __shared__ __attribute__((aligned(16))) float H1[R2 * LD];
  __shared__ float xs[R2 * NIN], red[4][R2];
  __shared__ double ys[R2], rs[R2], rm[R2], rc[R2];
  const int tid = threadIdx.x;
  const float* P = e.P;
  double sse = 0.0, mg = -INFINITY, cn = 0.0;
  for (int blk = blockIdx.x; blk < e.nblk; blk += gridDim.x) {
    const long long row0 = (long long)blk * R2;
    if (tid < R2 * NIN) {
      const long long row = min(row0 + tid / NIN, e.n - 1);
      xs[tid] = e.F[(size_t)row * e.ld + tid % NIN];
    } else if (tid >= 192 && tid < 192 + R2) {
      const long long row = min(row0 + (tid - 192), e.n - 1);
      ys[tid - 192] = e.y ? e.y[row] : (double)e.F[(size_t)row * e.ld + NIN];
    }
    __syncthreads();
    f4 acc[NT];
    forward_rows<NIN, HP, 1, Ly>(P, e.Wf, xs, H1, &red[0][0], acc);
    __syncthreads();
    if (tid < R2 && row0 + tid < e.n) {
      const float s = out_sum<1, 1>(&red[0][0], tid, 0);
      const float o = fmaxf(s + P[Ly::B2], 0.f);
      if (e.out) e.out[row0 + tid] = o;
      const double d = (double)o - ys[tid];
      sse += d * d;
      if (d > 0.0) {
        mg = fmax(mg, d / ys[tid]);
        cn += 1.0;
      }
    }
    __syncthreads();
  }
  if (tid < R2) {
    rs[tid] = sse;
    rm[tid] = mg;
    rc[tid] = cn;
  }
  __syncthreads();
  if (tid == 0) {
    for (int r = 1; r < R2; ++r) {
      sse += rs[r];
      mg = fmax(mg, rm[r]);
      cn += rc[r];
    }
    double* rec = e.part + 3 * (size_t)blockIdx.x;
    rec[0] = sse;
    rec[1] = mg;
    rec[2] = cn;
  }
}

// the workgroup records of k_eval in a fixed order; the margin of "no row above its target" is 0
__global__ __launch_bounds__(256) void k_eval_final(const double* part, int G, double* stats) {
  __shared__ double rs[256], rm[256], rc[256];
  const int tid = threadIdx.x;
  double sse = 0.0, mg = -INFINITY, cn = 0.0;
  for (int q = tid; q < G; q += 256) {
    sse += part[3 * q];
    mg = fmax(mg, part[3 * q + 1]);
    cn += part[3 * q + 2];
  }
  rs[tid] = sse;
  rm[tid] = mg;
  rc[tid] = cn;
  __syncthreads();
  if (tid == 0) {
    for (int r = 1; r < 256; ++r) {
      sse += rs[r];
      mg = fmax(mg, rm[r]);
      cn += rc[r];
    }
    stats[0] = sse;
    stats[1] = cn > 0.0 ? mg : 0.0;
    stats[2] = cn;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct vboc_fit {
  int nin, hidden, hp, bt, S;
  int total, rec;
  float *P = nullptr, *M = nullptr, *V = nullptr, *Wf = nullptr, *Wb = nullptr;
  float *H1p = nullptr, *dH2p = nullptr, *part = nullptr, *dW1p = nullptr;
  float* K = nullptr;                 // the pruning mask (padded layout); all real entries 1 while none is active
  bool masked = false;
  double* epart = nullptr;            // k_eval's records [EVG][3], then the three totals
  long long* npruned = nullptr;       // k_prune's count
  int* idx[2] = {nullptr, nullptr};
  State* st = nullptr;
  State* st_host = nullptr;           // pinned
  hipStream_t stream = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, t0 = nullptr, t1 = nullptr;
  hipGraphExec_t exec = nullptr;
  Args key{};
  int key_poll = 0;
  double last_ms = 0.0;
  long long last_launched = 0;
};

static thread_local std::string g_fit_err;
static int ffail(int code, const std::string& m) {
  g_fit_err = m;
  return code;
}
#define FCHK(x)                                                                         \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) return ffail(VBOC_FIT_EHIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

static void launch_sample(const vboc_fit*, const Args& a, hipStream_t s) {
  hipLaunchKernelGGL(k_sample, dim3(1), dim3(SNT), 0, s, a);
}

template <int NIN, int HP>
static void launch_train(const vboc_fit* h, const Args& a, hipStream_t s, bool fwd) {
  constexpr int NW1 = (HP / 32) * (HP / 32);
  const int nsmall = (Lay<NIN, HP>::SMALL + 15) / 16;
  if (fwd) {
    hipLaunchKernelGGL((k_fwd_bwd<NIN, HP>), dim3(h->bt / R2 + 1), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((k_dw1<NIN, HP>), dim3((HP / 64) * (HP / 64) * h->S), dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_adam<NIN, HP>), dim3(NW1 + nsmall), dim3(256), 0, s, a);
  }
}

static void train_part(const vboc_fit* h, const Args& a, hipStream_t s, bool fwd) {
  if (h->nin == 6 && h->hp == 512) launch_train<6, 512>(h, a, s, fwd);
  else if (h->nin == 4 && h->hp == 320) launch_train<4, 320>(h, a, s, fwd);
  else launch_train<2, 128>(h, a, s, fwd);
}

// Step i of a chunk uses the minibatch in idx[(parity + i) % 2], drawn by the previous step's forward kernel
// (or by the fit's first k_sample), and its forward kernel draws step i + 1's into the other buffer.
static void chunk(const vboc_fit* h, const Args& base, int steps, int parity, hipStream_t s) {
  for (int i = 0; i < steps; ++i) {
    Args a = base;
    a.idx = h->idx[(parity + i) & 1];
    a.idx_next = h->idx[(parity + i + 1) & 1];
    train_part(h, a, s, true);
    train_part(h, a, s, false);
  }
}

static bool supported(int nin, int hp) {
  return (nin == 6 && hp == 512) || (nin == 4 && hp == 320) || (nin == 2 && hp == 128);
}

template <int NIN, int HP>
static int total_of() { return Lay<NIN, HP>::TOTAL; }
template <int NIN, int HP>
static int rec_of() { return Lay<NIN, HP>::REC; }

static void pack(vboc_fit* h, float* W0, float* b0, float* W1, float* b1, float* W2, float* b2, int unpack,
                 float* src, bool frags = true) {
  const int nthr = h->hp * h->hp;
  dim3 g((nthr + 255) / 256), b(256);
  float *Wf = frags ? h->Wf : nullptr, *Wb = frags ? h->Wb : nullptr;
  if (h->nin == 6) hipLaunchKernelGGL((k_pack<6, 512>), g, b, 0, h->stream, src, Wf, Wb, W0, b0, W1, b1, W2, b2, h->hidden, unpack);
  else if (h->nin == 4) hipLaunchKernelGGL((k_pack<4, 320>), g, b, 0, h->stream, src, Wf, Wb, W0, b0, W1, b1, W2, b2, h->hidden, unpack);
  else hipLaunchKernelGGL((k_pack<2, 128>), g, b, 0, h->stream, src, Wf, Wb, W0, b0, W1, b1, W2, b2, h->hidden, unpack);
}

static LayR layr(const vboc_fit* h) {
  LayR L;
  L.nin = h->nin;
  L.hp = h->hp;
  L.H = h->hidden;
  L.b0 = h->hp * h->nin;
  L.b2 = L.b0 + 3 * h->hp;
  L.w1 = L.b2 + 4;
  L.total = h->total;
  return L;
}

// P = P * mask and the packed W1 fragments, on the trainer's stream
static void mask_apply(vboc_fit* h) {
  hipLaunchKernelGGL(k_mask_apply, dim3((h->total + 255) / 256), dim3(256), 0, h->stream, h->P, h->K, h->Wf, h->Wb,
                     layr(h));
}

template <int NIN, int HP>
static void launch_eval(const EvalArgs& e, int G, hipStream_t s) {
  hipLaunchKernelGGL((k_eval<NIN, HP>), dim3(G), dim3(256), 0, s, e);
}

extern "C" {

const char* vboc_fit_last_error(void) { return g_fit_err.c_str(); }

int vboc_fit_create(int nin, int hidden, int minibatch, unsigned long long seed, vboc_fit_handle* out) {
  if (!out) return ffail(VBOC_FIT_EARG, "out is null");
  *out = nullptr;
  const int hp = (hidden + 63) / 64 * 64;
  if (!supported(nin, hp))
    return ffail(VBOC_FIT_EUNSUPPORTED, "native fit supports (inputs, hidden) = (6, 449..512), (4, 257..320), "
                                        "(2, 65..128)");
  if (minibatch < 32 || minibatch % 32 || minibatch > MAXK)
    return ffail(VBOC_FIT_EUNSUPPORTED, "minibatch must be a multiple of 32 in [32, 4096]");
  vboc_fit* h = new vboc_fit();
  h->nin = nin;
  h->hidden = hidden;
  h->hp = hp;
  h->bt = minibatch;
  // split of the dW1 rows: about 256 workgroups, each split a multiple of 32 rows
  const int blocks = (hp / 64) * (hp / 64);
  int S = 1;
  while (blocks * S * 2 <= 256 && (minibatch / (S * 2)) % 32 == 0) S *= 2;
  h->S = S;
  if (nin == 6) { h->total = total_of<6, 512>(); h->rec = rec_of<6, 512>(); }
  else if (nin == 4) { h->total = total_of<4, 320>(); h->rec = rec_of<4, 320>(); }
  else { h->total = total_of<2, 128>(); h->rec = rec_of<2, 128>(); }
  auto fail_free = [&](hipError_t e, const char* what) {
    vboc_fit_destroy(h);
    return ffail(VBOC_FIT_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  hipError_t e;
#define FALLOC(ptr, bytes) \
  if ((e = hipMalloc((void**)&(ptr), (bytes))) != hipSuccess) return fail_free(e, "hipMalloc " #ptr)
  FALLOC(h->P, sizeof(float) * h->total);
  FALLOC(h->M, sizeof(float) * h->total);
  FALLOC(h->V, sizeof(float) * h->total);
  FALLOC(h->Wf, sizeof(float) * hp * hp);
  FALLOC(h->Wb, sizeof(float) * hp * hp);
  FALLOC(h->idx[0], sizeof(int) * minibatch);
  FALLOC(h->idx[1], sizeof(int) * minibatch);
  FALLOC(h->H1p, sizeof(float) * (size_t)hp * minibatch);
  FALLOC(h->dH2p, sizeof(float) * (size_t)hp * minibatch);
  FALLOC(h->part, sizeof(float) * (size_t)(minibatch / R2) * h->rec);
  FALLOC(h->dW1p, sizeof(float) * (size_t)S * hp * hp);
  FALLOC(h->st, sizeof(State));
  FALLOC(h->K, sizeof(float) * h->total);
  FALLOC(h->epart, sizeof(double) * 3 * (EVG + 1));
  FALLOC(h->npruned, sizeof(long long));
#undef FALLOC
  if ((e = hipHostMalloc((void**)&h->st_host, sizeof(State))) != hipSuccess) return fail_free(e, "hipHostMalloc");
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail_free(e, "stream");
  if ((e = hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming)) != hipSuccess) return fail_free(e, "event");
  if ((e = hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming)) != hipSuccess) return fail_free(e, "event");
  if ((e = hipEventCreate(&h->t0)) != hipSuccess) return fail_free(e, "event");
  if ((e = hipEventCreate(&h->t1)) != hipSuccess) return fail_free(e, "event");
  (void)hipMemsetAsync(h->P, 0, sizeof(float) * h->total, h->stream);
  (void)hipMemsetAsync(h->M, 0, sizeof(float) * h->total, h->stream);
  (void)hipMemsetAsync(h->V, 0, sizeof(float) * h->total, h->stream);
  (void)hipMemsetAsync(h->Wf, 0, sizeof(float) * hp * hp, h->stream);
  (void)hipMemsetAsync(h->Wb, 0, sizeof(float) * hp * hp, h->stream);
  const LayR L = layr(h);
  hipLaunchKernelGGL(k_mask_ones, dim3((h->total + 255) / 256), dim3(256), 0, h->stream, h->K, L);
  State s{};
  s.seed = seed;
  *h->st_host = s;
  (void)hipMemcpyAsync(h->st, h->st_host, sizeof(State), hipMemcpyHostToDevice, h->stream);
  if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail_free(e, "init");
  *out = h;
  return 0;
}

int vboc_fit_destroy(vboc_fit_handle h) {
  if (!h) return 0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->exec) (void)hipGraphExecDestroy(h->exec);
  float* bufs[] = {h->P, h->M, h->V, h->Wf, h->Wb, h->H1p, h->dH2p, h->part, h->dW1p, h->K};
  for (float* b : bufs)
    if (b) (void)hipFree(b);
  for (int* b : h->idx)
    if (b) (void)hipFree(b);
  if (h->st) (void)hipFree(h->st);
  if (h->epart) (void)hipFree(h->epart);
  if (h->npruned) (void)hipFree(h->npruned);
  if (h->st_host) (void)hipHostFree(h->st_host);
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
  if (h->ev_out) (void)hipEventDestroy(h->ev_out);
  if (h->t0) (void)hipEventDestroy(h->t0);
  if (h->t1) (void)hipEventDestroy(h->t1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int vboc_fit_set_params(vboc_fit_handle h, const float* W0, const float* b0, const float* W1, const float* b1,
                        const float* W2, const float* b2, void* stream) {
  if (!h || !W0 || !b0 || !W1 || !b1 || !W2 || !b2) return ffail(VBOC_FIT_EARG, "null argument");
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  pack(h, const_cast<float*>(W0), const_cast<float*>(b0), const_cast<float*>(W1), const_cast<float*>(b1),
       const_cast<float*>(W2), const_cast<float*>(b2), 0, h->P);
  if (h->masked) mask_apply(h);
  FCHK(hipGetLastError());
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  return 0;
}

int vboc_fit_get_params(vboc_fit_handle h, int which, float* W0, float* b0, float* W1, float* b1, float* W2,
                        float* b2, void* stream) {
  if (!h || !W0 || !b0 || !W1 || !b1 || !W2 || !b2) return ffail(VBOC_FIT_EARG, "null argument");
  if (which < 0 || which > 2) return ffail(VBOC_FIT_EARG, "which: 0 parameters, 1 exp_avg, 2 exp_avg_sq");
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  pack(h, W0, b0, W1, b1, W2, b2, 1, which == 0 ? h->P : which == 1 ? h->M : h->V);
  FCHK(hipGetLastError());
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  return 0;
}

int vboc_fit_train(vboc_fit_handle h, const vboc_fit_run_t* r, void* stream) {
  if (!h || !r || !r->F) return ffail(VBOC_FIT_EARG, "null argument");
  if (r->ld < h->nin + 1) return ffail(VBOC_FIT_EARG, "ld < inputs + 1");
  if (r->n_new == 0 && r->n < h->bt) return ffail(VBOC_FIT_EARG, "fewer rows than one minibatch");
  if (r->n_new != 0 && (r->n_new < h->bt / 2 || r->n - r->n_new < h->bt / 2 || r->n_new > r->n))
    return ffail(VBOC_FIT_EARG, "a refit needs at least minibatch/2 old and new rows");
  if (r->n >= (1ll << 31)) return ffail(VBOC_FIT_EARG, "more than 2^31 rows");
  if (r->it_max < 1) return ffail(VBOC_FIT_EARG, "it_max < 1");
  // a graph replays an even number of steps, so every replay starts on idx[0]
  const int poll = r->graphs ? (r->poll > 2 ? (r->poll + 1) / 2 * 2 : 2) : (r->poll > 0 ? r->poll : 1);
  Args a;
  memset(&a, 0, sizeof a);
  a.P = h->P; a.M = h->M; a.V = h->V; a.K = h->masked ? h->K : nullptr; a.Wf = h->Wf; a.Wb = h->Wb; a.idx = nullptr;
  a.H1p = h->H1p; a.dH2p = h->dH2p; a.part = h->part; a.dW1p = h->dW1p; a.st = h->st;
  a.F = r->F; a.n = r->n; a.n_new = r->n_new; a.ldF = r->ld; a.Bt = h->bt; a.S = h->S; a.lr = (float)r->lr;
  // loop state of the reference: it = 1, val = max |qdot| of the training rows (given by the caller in f64)
  FCHK(hipStreamSynchronize(h->stream));
  State* s = h->st_host;
  FCHK(hipMemcpyAsync(s, h->st, sizeof(State), hipMemcpyDeviceToHost, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  s->val = r->val0;
  s->stop = r->stop_val;
  s->beta = r->beta;
  s->it = 1;
  s->it_lim = r->it_max;
  s->gate = 1;
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  FCHK(hipMemcpyAsync(h->st, s, sizeof(State), hipMemcpyHostToDevice, h->stream));
  const unsigned long long d0 = s->draws;
  // the first step's minibatch (draw d0); every later one is drawn beside the step before it
  Args a0 = a;
  a0.idx = h->idx[0];
  launch_sample(h, a0, h->stream);
  FCHK(hipGetLastError());
  const bool same = h->exec && h->key_poll == poll && memcmp(&h->key, &a, sizeof(Args)) == 0;
  if (r->graphs && !same) {
    if (h->exec) {
      (void)hipGraphExecDestroy(h->exec);
      h->exec = nullptr;
    }
    hipGraph_t g;
    FCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    chunk(h, a, poll, 0, h->stream);
    FCHK(hipStreamEndCapture(h->stream, &g));
    hipError_t e = hipGraphInstantiate(&h->exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return ffail(VBOC_FIT_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    h->key = a;
    h->key_poll = poll;
  }
  FCHK(hipEventRecord(h->t0, h->stream));
  long long launched = 0;
  for (;;) {
    if (r->graphs) FCHK(hipGraphLaunch(h->exec, h->stream));
    else chunk(h, a, poll, (int)(launched & 1), h->stream);
    FCHK(hipGetLastError());
    launched += poll;
    FCHK(hipMemcpyAsync(&s->gate, &h->st->gate, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    FCHK(hipStreamSynchronize(h->stream));
    if (!s->gate) break;
    if (launched > r->it_max + poll) return ffail(VBOC_FIT_EHIP, "fit did not stop at it_max");
  }
  FCHK(hipEventRecord(h->t1, h->stream));
  FCHK(hipMemcpyAsync(s, h->st, sizeof(State), hipMemcpyDeviceToHost, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  // the sampler stream continues after the steps taken (the ones drawn past the stop are dropped), so the next
  // fit draws what a step-by-step loop would
  s->draws = d0 + (unsigned long long)(s->it - 1);
  FCHK(hipMemcpyAsync(&h->st->draws, &s->draws, sizeof(s->draws), hipMemcpyHostToDevice, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, h->t0, h->t1);
  h->last_ms = ms;
  h->last_launched = launched;
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  if (r->iterations) *r->iterations = s->it - 1;
  if (r->val) *r->val = s->val;
  if (r->launched) *r->launched = launched;
  if (r->kernel_ms) *r->kernel_ms = ms;
  return 0;
}

int vboc_fit_sample(vboc_fit_handle h, long long n, long long n_new, int steps, int* idx_out, void* stream) {
  if (!h || !idx_out || steps < 0) return ffail(VBOC_FIT_EARG, "bad argument");
  if (n_new == 0 && n < h->bt) return ffail(VBOC_FIT_EARG, "fewer rows than one minibatch");
  if (n_new != 0 && (n_new < h->bt / 2 || n - n_new < h->bt / 2 || n_new > n))
    return ffail(VBOC_FIT_EARG, "a refit needs at least minibatch/2 old and new rows");
  if (n >= (1ll << 31)) return ffail(VBOC_FIT_EARG, "more than 2^31 rows");
  FCHK(hipStreamSynchronize(h->stream));
  State* s = h->st_host;
  FCHK(hipMemcpyAsync(s, h->st, sizeof(State), hipMemcpyDeviceToHost, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  const State keep = *s;
  s->val = 1.0;
  s->stop = 0.0;
  s->it = 1;
  s->it_lim = 1ll << 62;
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  FCHK(hipMemcpyAsync(h->st, s, sizeof(State), hipMemcpyHostToDevice, h->stream));
  Args a;
  memset(&a, 0, sizeof a);
  a.idx = h->idx[0]; a.st = h->st;
  a.n = n; a.n_new = n_new; a.ldF = 0; a.Bt = h->bt; a.S = h->S;
  for (int i = 0; i < steps; ++i) {
    launch_sample(h, a, h->stream);
    FCHK(hipGetLastError());
    FCHK(hipMemcpyAsync(idx_out + (size_t)i * h->bt, h->idx[0], sizeof(int) * h->bt, hipMemcpyDeviceToDevice,
                        h->stream));
  }
  FCHK(hipMemcpyAsync(s, h->st, sizeof(State), hipMemcpyDeviceToHost, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  State back = keep;
  back.draws = s->draws;
  *s = back;
  FCHK(hipMemcpyAsync(h->st, s, sizeof(State), hipMemcpyHostToDevice, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  return 0;
}

int vboc_fit_info(vboc_fit_handle h, int* hidden_padded, int* splits, long long* adam_steps,
                  unsigned long long* draws) {
  if (!h) return ffail(VBOC_FIT_EARG, "null handle");
  FCHK(hipStreamSynchronize(h->stream));
  FCHK(hipMemcpyAsync(h->st_host, h->st, sizeof(State), hipMemcpyDeviceToHost, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  const State s = *h->st_host;
  if (hidden_padded) *hidden_padded = h->hp;
  if (splits) *splits = h->S;
  if (adam_steps) *adam_steps = s.step_t;
  if (draws) *draws = s.draws;
  return 0;
}

int vboc_fit_set_mask(vboc_fit_handle h, const float* W0, const float* b0, const float* W1, const float* b1,
                      const float* W2, const float* b2, void* stream) {
  if (!h) return ffail(VBOC_FIT_EARG, "null handle");
  const int given = !!W0 + !!b0 + !!W1 + !!b1 + !!W2 + !!b2;
  if (given != 0 && given != 6) return ffail(VBOC_FIT_EARG, "give all six masks, or none to remove the mask");
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  if (given) {
    pack(h, const_cast<float*>(W0), const_cast<float*>(b0), const_cast<float*>(W1), const_cast<float*>(b1),
         const_cast<float*>(W2), const_cast<float*>(b2), 0, h->K, false);
    mask_apply(h);
  } else {
    hipLaunchKernelGGL(k_mask_ones, dim3((h->total + 255) / 256), dim3(256), 0, h->stream, h->K, layr(h));
  }
  FCHK(hipGetLastError());
  h->masked = given != 0;
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  return 0;
}

int vboc_fit_get_mask(vboc_fit_handle h, float* W0, float* b0, float* W1, float* b1, float* W2, float* b2,
                      void* stream) {
  if (!h || !W0 || !b0 || !W1 || !b1 || !W2 || !b2) return ffail(VBOC_FIT_EARG, "null argument");
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  pack(h, W0, b0, W1, b1, W2, b2, 1, h->K);
  FCHK(hipGetLastError());
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  return 0;
}

int vboc_fit_prune(vboc_fit_handle h, long long nprune, long long* pruned, void* stream) {
  if (!h) return ffail(VBOC_FIT_EARG, "null handle");
  if (h->masked) return ffail(VBOC_FIT_EARG, "a mask is already active (remove it first)");
  const long long H = h->hidden, n = H * h->nin + H + H * H + H + H + 1;
  if (nprune < 0 || nprune > n) return ffail(VBOC_FIT_EARG, "nprune outside [0, parameter count]");
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  hipLaunchKernelGGL(k_prune, dim3(1), dim3(PNT), 0, h->stream, h->P, h->K, layr(h), nprune, h->npruned);
  mask_apply(h);
  FCHK(hipGetLastError());
  long long got = -1;
  FCHK(hipMemcpyAsync(&got, h->npruned, sizeof got, hipMemcpyDeviceToHost, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  h->masked = true;
  if (pruned) *pruned = got;
  if (got != nprune) return ffail(VBOC_FIT_EHIP, "the selection pruned " + std::to_string(got) + " entries");
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  return 0;
}

int vboc_fit_eval(vboc_fit_handle h, const float* F, long long n, int ld, const double* y, float* out,
                  double* stats, void* stream) {
  if (!h || !stats) return ffail(VBOC_FIT_EARG, "null argument");
  if (n < 0 || n >= (1ll << 31)) return ffail(VBOC_FIT_EARG, "rows outside [0, 2^31)");
  stats[0] = stats[1] = stats[2] = 0.0;
  if (n == 0) return 0;
  if (!F) return ffail(VBOC_FIT_EARG, "null argument");
  if (ld < h->nin + (y ? 0 : 1)) return ffail(VBOC_FIT_EARG, "ld < inputs (+ 1 for the target column)");
  EvalArgs e;
  e.P = h->P; e.Wf = h->Wf; e.F = F; e.y = y; e.out = out; e.part = h->epart; e.n = n; e.ld = ld;
  e.nblk = (int)((n + R2 - 1) / R2);
  const int G = e.nblk < EVG ? e.nblk : EVG;
  FCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  FCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
  if (h->nin == 6) launch_eval<6, 512>(e, G, h->stream);
  else if (h->nin == 4) launch_eval<4, 320>(e, G, h->stream);
  else launch_eval<2, 128>(e, G, h->stream);
  double* tot = h->epart + 3 * (size_t)EVG;
  hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(256), 0, h->stream, h->epart, G, tot);
  FCHK(hipGetLastError());
  FCHK(hipMemcpyAsync(stats, tot, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  FCHK(hipStreamSynchronize(h->stream));
  FCHK(hipEventRecord(h->ev_out, h->stream));
  FCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  return 0;
}

}  // extern "C"
