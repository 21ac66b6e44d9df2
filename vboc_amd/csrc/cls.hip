// The classifier of the HJR (and AL) loops on the device: Adam / BCEWithLogitsLoss training of NeuralNetCLS
// (Linear-ReLU-Linear-ReLU-Linear, two logits) with the reference's minibatch sampling and stop rule, the
// classification of a candidate set, and the RMSE march along each held-out state's velocity direction.  The training
// kernels are templates over <inputs, padded hidden> and exist at hidden 128 (HJR: inputs 2, 4, 6) and, as fit.hip's,
// at (4, 320) and (6, 512) (the AL loop's 300 and 500); the forward-only kernels exist at 128 alone (the AL loop
// classifies and marches on pool.hip).
//
// Reference: HJR/triplependulum_hjr.py:95-118 and :234-258 (random.sample(range(n), 4096), BCEWithLogitsLoss,
// Adam(lr 1e-3), val = beta val + (1 - beta) loss from val = 1, `while val > loss_stop and it < it_max`), :136-148
// and :203-213 (argmax over a candidate set), :150-176 (the march), my_nn.py:4-18 (the model), the double /
// pendulum twins.  The training step keeps fit.hip's structure (one step = three kernels, `poll` steps per graph):
//
//   k_fwd_bwd   the step's gate; one extra workgroup draws the NEXT step's minibatch; 16 minibatch rows per other
//               workgroup: H1 = relu(x W0' + b0), H2 = relu(H1 W1' + b1) and dH1 = (dH2 W1) * [H1 > 0] on
//               v_mfma_f32_16x16x4_f32, the two logits, the BCE loss and gradient, per-workgroup partial gradients
//   k_dw1       dW1 = dH2' H1 (split over minibatch rows), plus the EMA / counter update of the reference's loop
//   k_adam      the partial sums reduced in a fixed order, torch.optim.Adam's update, W1 repacked as MFMA fragments
//
// k_eval is the forward pass alone (labels, logits, the count of label 1); k_boundary marches one ray per
// workgroup, 16 steps per round through the same forward pass.  There is one forward pass: nn_common.h's forward_rows,
// called by k_fwd_bwd (which also packs H1 for dW1) and by forward16 (k_eval, k_boundary).  Every reduction has a
// fixed order; a step whose gate is 0 changes nothing; every loop has a static bound (the sampler's probes end because
// its table is half empty).  Hidden units 100..127 of the padded buffers stay exactly zero: their gradients are exact
// zeros.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/vboc_cls.h"
#include "nn_common.h"

namespace {

constexpr int HPF = 128;      // padded hidden size of the forward-only kernels (k_eval, k_boundary)
constexpr int R2 = 16;        // rows per workgroup and round
constexpr int EVG = 2048;     // most workgroups (= partial counts) of one evaluation
constexpr int MAX_STEPS = 16384;

struct State {
  double val, stop, beta;
  long long it, it_lim, step_t;
  unsigned long long draws, seed;
  int gate, err, pad0, pad1;
};

struct Args {
  float* P;                   // parameters: [W0 (HP x NIN) | b0 | b1 | W2 (2 x HP) | b2 (4) | W1 (HP x HP)]
  float* M;                   // Adam exp_avg, same layout
  float* V;                   // Adam exp_avg_sq
  float* Wf;                  // W1 packed as the forward product's B fragments: pk(j, k, HP / 16)
  float* Wb;                  // W1 packed as the backward product's B fragments: element W1[j][c] at pk(c, j, HP / 16)
  int* idx;                   // this step's minibatch row indices [Bt]
  int* idx_next;              // the next step's, drawn by the forward kernel's extra workgroup
  float* H1p;                 // H1 packed as dW1's B fragments: element H1[r][c] at pk(c, r, Bt / 16)
  float* dH2p;                // dH2 packed as dW1's A fragments: element dH2[r][j] at pk(j, r, Bt / 16)
  float* part;                // per-workgroup partials [Bt / R2][REC]
  float* dW1p;                // split partials of dW1 [S][HP][HP]
  State* st;
  const float* F;             // rows [n][ldF]: NIN normalised inputs then the two targets
  long long n, n_new;         // n_new > 0: the last n_new rows are the new ones (half of each minibatch from them)
  int ldF, Bt, S;
  float lr;
};

template <int NIN, int HP>
struct Lay {
  static constexpr int W0 = 0, B0 = HP * NIN, B1 = B0 + HP, W2 = B1 + HP, B2 = W2 + 2 * HP, SMALL = B2 + 4;
  static constexpr int W1 = SMALL, TOTAL = W1 + HP * HP, REC = SMALL + 4, LOSS = SMALL;
};

// the first minibatch of a fit (and the test hook vboc_cls_sample), into a.idx
__global__ __launch_bounds__(SNT) void k_sample(Args a) {
  __shared__ SampLds L;
  sample_minibatch(L, a, a.idx);
}

template <int NIN, int HP>
__global__ __launch_bounds__(256) void k_fwd_bwd(Args a) {
  using Ly = Lay<NIN, HP>;
  constexpr int NT = HP / 64;          // 16-column tiles per wave
  constexpr int LD = HP + 4;           // LDS row stride of the activations
  struct FwdLds {
    float H1[R2 * LD];
    float G2[R2 * LD];
    float xs[R2 * NIN], ys[R2 * 2], dout[R2 * 2], ls[R2 * 2], red[4][R2][2];
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
  float* ls = U.f.ls;
  // the step's gate (the reference's `while val > loss_stop and it < it_max`), from the state the previous step
  // left; block 0 publishes it for this step's dW1 / Adam kernels and the host's poll
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
  if (tid < R2 * (NIN + 2)) {
    const int r = tid / (NIN + 2), i = tid % (NIN + 2);
    const float v = a.F[(size_t)a.idx[row0 + r] * a.ldF + i];
    if (i < NIN) xs[r * NIN + i] = v;
    else ys[r * 2 + i - NIN] = v;
  }
  __syncthreads();

  // the forward pass; H1 is also written transposed for dW1.  acc[u][g] = H2[row 4 lq + g][col 16 (w + 4u) + lr]
  f4 acc[NT];
  auto pack_h1 = [&](int c, const float(&h)[R2]) {
    f4* dst = (f4*)(a.H1p + pk(c, row0, a.Bt / 16));
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[16 * q] = f4{h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]};
  };
  forward_rows<NIN, HP, 2, Ly>(P, a.Wf, xs, H1, &U.f.red[0][0][0], acc, pack_h1);
  __syncthreads();
  if (tid < 2 * R2) {
    const int r = tid >> 1, o = tid & 1;
    const float s = out_sum<2, 1>(&U.f.red[0][0][0], r, o);
    const float x = s + P[Ly::B2 + o], y = ys[tid];
    // BCEWithLogitsLoss, mean over 2 Bt elements: max(x, 0) - x y + log1p(exp(-|x|)); d / dx = (sigmoid(x) - y) / (2 Bt)
    ls[tid] = (fmaxf(x, 0.f) - x * y) + log1pf(expf(-fabsf(x)));
    dout[tid] = (1.f / (1.f + expf(-x)) - y) / (float)(2 * a.Bt);
  }
  __syncthreads();

  float* part = a.part + (size_t)blockIdx.x * Ly::REC;
  float d0[4], d1[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    d0[g] = dout[2 * (4 * lq + g)];
    d1[g] = dout[2 * (4 * lq + g) + 1];
  }
  // dH2 = (dout W2) [H2 > 0]; db1 and dW2 partials; dH2 to LDS and transposed to global
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int j = 16 * (w + 4 * u) + lr;
    const float w0 = P[Ly::W2 + j], w1 = P[Ly::W2 + HP + j];
    float gv[4], sb = 0.f, s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float h = acc[u][g];
      gv[g] = h > 0.f ? fmaf(d1[g], w1, d0[g] * w0) : 0.f;
      sb += gv[g];
      s0 = fmaf(d0[g], h, s0);
      s1 = fmaf(d1[g], h, s1);
      G2[(4 * lq + g) * LD + j] = gv[g];
    }
    *(f4*)(a.dH2p + pk(j, row0 + 4 * lq, a.Bt / 16)) = f4{gv[0], gv[1], gv[2], gv[3]};
    sb += __shfl_xor(sb, 16);
    sb += __shfl_xor(sb, 32);
    s0 += __shfl_xor(s0, 16);
    s0 += __shfl_xor(s0, 32);
    s1 += __shfl_xor(s1, 16);
    s1 += __shfl_xor(s1, 32);
    if (lq == 0) {
      part[Ly::B1 + j] = sb;
      part[Ly::W2 + j] = s0;
      part[Ly::W2 + HP + j] = s1;
    }
  }
  if (tid == 0) {
    float s0 = 0.f, s1 = 0.f, l = 0.f;
    for (int r = 0; r < R2; ++r) {
      s0 += dout[2 * r];
      s1 += dout[2 * r + 1];
      l += ls[2 * r];
      l += ls[2 * r + 1];
    }
    part[Ly::B2] = s0;
    part[Ly::B2 + 1] = s1;
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
  const int T = KC / 16;      // KC is a multiple of 32
  for (int t = 0; t < T; ++t) {
    const f4 av[2] = {*(const f4*)(A0 + 256 * t), *(const f4*)(A1 + 256 * t)};
    const f4 bv[2] = {*(const f4*)(B0 + 256 * t), *(const f4*)(B1 + 256 * t)};
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        acc[x][y] = mfma(av[x].x, bv[y].x, acc[x][y]);
        acc[x][y] = mfma(av[x].y, bv[y].y, acc[x][y]);
        acc[x][y] = mfma(av[x].z, bv[y].z, acc[x][y]);
        acc[x][y] = mfma(av[x].w, bv[y].w, acc[x][y]);
      }
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
      const float loss = l / (float)(2 * a.Bt);
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
      float p = a.P[Ly::W1 + o], m = a.M[Ly::W1 + o], v = a.V[Ly::W1 + o];
      adam(p, m, v, g, k);
      a.P[Ly::W1 + o] = p;
      a.M[Ly::W1 + o] = m;
      a.V[Ly::W1 + o] = v;
      tile[rj][rc] = p;
    }
    __syncthreads();
    // the new W1 tile as the packed B fragments of both products: 4 blocks of 16 x 16, lane-major
    constexpr int TG = HP / 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q, bi = e >> 8, L = (e >> 2) & 63, sx = e & 3;
      const int b_r = bi >> 1, b_c = bi & 1, lr = L & 15, lq = L >> 4;
      a.Wf[(((size_t)(tj * 2 + b_r) * TG + tc * 2 + b_c) * 64 + L) * 4 + sx] = tile[16 * b_r + lr][16 * b_c + 4 * lq + sx];
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
    float p = a.P[e], m = a.M[e], v = a.V[e];
    adam(p, m, v, s, k);
    a.P[e] = p;
    a.M[e] = m;
    a.V[e] = v;
  }
}

// torch layouts <-> padded buffers (H real hidden units)
template <int NIN, int HP>
__global__ void k_pack(float* P, float* Wf, float* Wb, float* W0, float* b0, float* W1, float* b1, float* W2,
                       float* b2, int H, int unpack) {
  using Ly = Lay<NIN, HP>;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < HP * HP) {
    const int j = i / HP, c = i % HP;
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
    const int c = i;
    if (unpack) {
      if (c < H) {
        for (int q = 0; q < NIN; ++q) W0[c * NIN + q] = P[Ly::W0 + c * NIN + q];
        b0[c] = P[Ly::B0 + c];
        b1[c] = P[Ly::B1 + c];
        W2[c] = P[Ly::W2 + c];
        W2[H + c] = P[Ly::W2 + HP + c];
      }
      if (c < 2) b2[c] = P[Ly::B2 + c];
    } else {
      for (int q = 0; q < NIN; ++q) P[Ly::W0 + c * NIN + q] = c < H ? W0[c * NIN + q] : 0.f;
      P[Ly::B0 + c] = c < H ? b0[c] : 0.f;
      P[Ly::B1 + c] = c < H ? b1[c] : 0.f;
      P[Ly::W2 + c] = c < H ? W2[c] : 0.f;
      P[Ly::W2 + HP + c] = c < H ? W2[H + c] : 0.f;
      if (c < 4) P[Ly::B2 + c] = c < 2 ? b2[c] : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// the forward pass alone: classification and the march
// ------------------------------------------------------------------------------------------------
struct FwdOnlyLds {
  float H1[R2 * (HPF + 4)];
  float xs[R2 * 6];
  float red[4][R2][2];
  float lg[R2][2];
};

// The two logits of the 16 rows in L.xs (normalised inputs, written and barrier-synchronised by the caller) into
// L.lg, through the training forward's own code (forward_rows).  Called by all 256 threads; ends on a barrier.
template <int NIN>
__device__ __forceinline__ void forward16(const float* P, const float* Wf, FwdOnlyLds& L) {
  using Ly = Lay<NIN, HPF>;
  const int tid = threadIdx.x;
  f4 acc[HPF / 64];
  forward_rows<NIN, HPF, 2, Ly>(P, Wf, L.xs, L.H1, &L.red[0][0][0], acc);
  __syncthreads();
  if (tid < 2 * R2) {
    const int r = tid >> 1, o = tid & 1;
    L.lg[r][o] = out_sum<2, 1>(&L.red[0][0][0], r, o) + P[Ly::B2 + o];
  }
  __syncthreads();
}

struct EvalArgs {
  const float* P;
  const float* Wf;
  const float* X;             // rows [n][ld]: NIN normalised inputs
  unsigned char* labels;      // [n]
  float* logits;              // [n][2], or null
  int* part;                  // per-workgroup counts of label 1 [gridDim.x]
  long long n;
  int ld, nblk;
};

// 16 contiguous rows per workgroup and round; the last block's rows are loaded with clamped indices and masked on
// output.  Thread r < 16 counts row r's labels over the workgroup's blocks, thread 0 adds the 16.
template <int NIN>
__global__ __launch_bounds__(256) void k_eval(EvalArgs e) {
  __shared__ __attribute__((aligned(16))) FwdOnlyLds L;
  __shared__ int cs[R2];
  const int tid = threadIdx.x;
  int cnt = 0;
  for (int blk = blockIdx.x; blk < e.nblk; blk += gridDim.x) {
    const long long row0 = (long long)blk * R2;
    if (tid < R2 * NIN) {
      const long long row = min(row0 + tid / NIN, e.n - 1);
      L.xs[tid] = e.X[(size_t)row * e.ld + tid % NIN];
    }
    __syncthreads();
    forward16<NIN>(e.P, e.Wf, L);
    if (tid < R2 && row0 + tid < e.n) {
      const float l0 = L.lg[tid][0], l1 = L.lg[tid][1];
      const int lab = l1 > l0;          // a tie is 0, as np.argmax
      e.labels[row0 + tid] = (unsigned char)lab;
      if (e.logits) {
        e.logits[2 * (row0 + tid)] = l0;
        e.logits[2 * (row0 + tid) + 1] = l1;
      }
      cnt += lab;
    }
  }
  if (tid < R2) cs[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    for (int r = 1; r < R2; ++r) cnt += cs[r];
    e.part[blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(256) void k_count_final(const int* part, int G, long long* total) {
  __shared__ long long rs[256];
  const int tid = threadIdx.x;
  long long c = 0;
  for (int q = tid; q < G; q += 256) c += part[q];
  rs[tid] = c;
  __syncthreads();
  if (tid == 0) {
    for (int r = 1; r < 256; ++r) c += rs[r];
    *total = c;
  }
}

struct MarchArgs {
  const float* P;
  const float* Wf;
  const double* X;            // held-out states [m][NIN]
  double* err;                // [m]
  int* steps;                 // [m]
  unsigned char* flags;       // [m]
  float mean, std;
  int max_steps;
};

// One ray per workgroup (HJR/triplependulum_hjr.py:150-176).  Round 0 classifies the start point; every later round
// classifies the next 16 points of the ray: thread r < 16 forms point base + r + 1 from the round's base velocity
// (nn_common.h's ray helpers, shared with pool.hip's march), casts it to float32 and normalises it in float32.  The
// first point whose label differs, whose |v| <= 1e-2 or whose index is max_steps ends the march.
template <int NIN>
__global__ __launch_bounds__(256) void k_boundary(MarchArgs a) {
  constexpr int NQ = NIN / 2;
  __shared__ __attribute__((aligned(16))) FwdOnlyLds L;
  __shared__ double vb[NQ];
  __shared__ int stop[R2];
  const int tid = threadIdx.x, ray = blockIdx.x;
  const double* x = a.X + (size_t)ray * NIN;
  double v0[NQ], c[NQ], v[NQ], sn;
#pragma unroll
  for (int i = 0; i < NQ; ++i) v0[i] = x[NQ + i];
  const double vel_norm = ray_norm<NQ, true>(v0, 0, false, sn);
  // the start label, from the float32 cast of the row
  if (tid < R2 * NIN) L.xs[tid] = ((float)x[tid % NIN] - a.mean) / a.std;
  if (tid < NQ) vb[tid] = v0[tid];
  __syncthreads();
  forward16<NIN>(a.P, a.Wf, L);
  const int label = L.lg[0][1] > L.lg[0][0];
#pragma unroll
  for (int i = 0; i < NQ; ++i) c[i] = ray_step(v0[i], vel_norm, label);
  float xq[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) xq[i] = ((float)x[i] - a.mean) / a.std;
  if (vel_norm > 1e-2) {
    const int rounds = (a.max_steps + R2 - 1) / R2;
    int done = 0;
    for (int rd = 0; rd < rounds && !done; ++rd) {
      const int base = rd * R2;
      double vn = 0.0;
      if (tid < R2) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) v[i] = vb[i];
        ray_point<NQ>(v, c, tid);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          L.xs[tid * NIN + i] = xq[i];
          L.xs[tid * NIN + NQ + i] = ((float)v[i] - a.mean) / a.std;
        }
        vn = ray_norm<NQ, true>(v, 0, false, sn);
      }
      __syncthreads();
      forward16<NIN>(a.P, a.Wf, L);
      if (tid < R2) {
        const int out = L.lg[tid][1] > L.lg[tid][0];
        const int s = base + tid + 1;
        stop[tid] = (out != label) | ((!(vn > 1e-2)) << 1) | ((s >= a.max_steps) << 2);
      }
      __syncthreads();
      int first = R2;
      for (int r = R2 - 1; r >= 0; --r)
        if (stop[r]) first = r;
      if (first < R2) {
        done = 1;
        if (tid == first) {
          a.err[ray] = vel_norm - vn;
          a.steps[ray] = base + first + 1;
          a.flags[ray] = (unsigned char)(label | ((stop[first] == 4) << 1));   // bit 1: stopped by max_steps alone
        }
      } else if (tid == R2 - 1) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) vb[i] = v[i];
      }
      __syncthreads();
    }
    return;       // the last round's points include index max_steps, so a round has ended the ray
  }
  // no step taken (|v_test| <= 1e-2)
  if (tid == 0) {
    a.err[ray] = 0.0;
    a.steps[ray] = 0;
    a.flags[ray] = (unsigned char)label;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct vboc_cls {
  int nin, hidden, hp, bt, S;
  int total, rec;
  float *P = nullptr, *M = nullptr, *V = nullptr, *Wf = nullptr, *Wb = nullptr;
  float *H1p = nullptr, *dH2p = nullptr, *part = nullptr, *dW1p = nullptr;
  int* epart = nullptr;               // k_eval's counts [EVG]
  long long* etotal = nullptr;
  int* idx[2] = {nullptr, nullptr};
  State* st = nullptr;
  State* st_host = nullptr;           // pinned
  hipStream_t stream = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, t0 = nullptr, t1 = nullptr;
  hipGraphExec_t exec = nullptr;
  Args key{};
  int key_poll = 0;
};

static thread_local std::string g_cls_err;
static int cfail(int code, const std::string& m) {
  g_cls_err = m;
  return code;
}
#define CCHK(x)                                                                         \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) return cfail(VBOC_CLS_EHIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

// The handle's instantiation <inputs, padded hidden>, as a tag: (2 | 4 | 6, 128), (4, 320) or (6, 512).
template <int NIN_, int HP_>
struct Shape {
  static constexpr int NIN = NIN_, HP = HP_;
};
template <class F>
static void with_shape(const vboc_cls* h, F&& f) {
  if (h->hp == 512) f(Shape<6, 512>{});
  else if (h->hp == 320) f(Shape<4, 320>{});
  else if (h->nin == 6) f(Shape<6, 128>{});
  else if (h->nin == 4) f(Shape<4, 128>{});
  else f(Shape<2, 128>{});
}

template <int NIN, int HP>
static void launch_train(const vboc_cls* h, const Args& a, hipStream_t s) {
  constexpr int NW1 = (HP / 32) * (HP / 32);
  const int nsmall = (Lay<NIN, HP>::SMALL + 15) / 16;
  hipLaunchKernelGGL((k_fwd_bwd<NIN, HP>), dim3(h->bt / R2 + 1), dim3(256), 0, s, a);
  hipLaunchKernelGGL((k_dw1<NIN, HP>), dim3((HP / 64) * (HP / 64) * h->S), dim3(256), 0, s, a);
  hipLaunchKernelGGL((k_adam<NIN, HP>), dim3(NW1 + nsmall), dim3(256), 0, s, a);
}

// Step i of a chunk uses the minibatch in idx[(parity + i) % 2], drawn by the previous step's forward kernel
// (or by the fit's first k_sample), and its forward kernel draws step i + 1's into the other buffer.
static void chunk(const vboc_cls* h, const Args& base, int steps, int parity, hipStream_t s) {
  for (int i = 0; i < steps; ++i) {
    Args a = base;
    a.idx = h->idx[(parity + i) & 1];
    a.idx_next = h->idx[(parity + i + 1) & 1];
    with_shape(h, [&](auto sh) { launch_train<decltype(sh)::NIN, decltype(sh)::HP>(h, a, s); });
  }
}

template <int NIN, int HP>
static void pack(vboc_cls* h, float* W0, float* b0, float* W1, float* b1, float* W2, float* b2, int unpack,
                 float* src) {
  hipLaunchKernelGGL((k_pack<NIN, HP>), dim3((HP * HP + 255) / 256), dim3(256), 0, h->stream, src, h->Wf, h->Wb, W0,
                     b0, W1, b1, W2, b2, h->hidden, unpack);
}

static void pack(vboc_cls* h, float* W0, float* b0, float* W1, float* b1, float* W2, float* b2, int unpack,
                 float* src) {
  with_shape(h, [&](auto sh) { pack<decltype(sh)::NIN, decltype(sh)::HP>(h, W0, b0, W1, b1, W2, b2, unpack, src); });
}

// a refit's row ranges: n_new = 0 is one range; else each half of the minibatch needs its range to hold it
static int check_rows(const vboc_cls* h, long long n, long long n_new) {
  if (n_new < 0 || n_new > n) return cfail(VBOC_CLS_EARG, "n_new outside [0, n]");
  if (n_new == 0 && n < h->bt) return cfail(VBOC_CLS_EARG, "fewer rows than one minibatch");
  if (n_new != 0 && (n_new < h->bt / 2 || n - n_new < h->bt / 2))
    return cfail(VBOC_CLS_EARG, "a split minibatch needs at least minibatch/2 old and minibatch/2 new rows");
  if (n >= (1ll << 31)) return cfail(VBOC_CLS_EARG, "more than 2^31 rows");
  return 0;
}

// the caller's stream waits for the classifier's, or the other way round
static int order(hipEvent_t ev, hipStream_t first, hipStream_t then) {
  CCHK(hipEventRecord(ev, first));
  CCHK(hipStreamWaitEvent(then, ev, 0));
  return 0;
}

extern "C" {

const char* vboc_cls_last_error(void) { return g_cls_err.c_str(); }

int vboc_cls_create(int nin, int hidden, int minibatch, unsigned long long seed, vboc_cls_handle* out) {
  if (!out) return cfail(VBOC_CLS_EARG, "out is null");
  *out = nullptr;
  const int hp = (hidden + 63) / 64 * 64;
  const bool narrow = (nin == 2 || nin == 4 || nin == 6) && hidden >= 65 && hidden <= 128;
  if (!narrow && !(nin == 4 && hp == 320) && !(nin == 6 && hp == 512))
    return cfail(VBOC_CLS_EUNSUPPORTED, "native classifier supports inputs 2, 4, 6 with hidden 65..128, and the fit "
                                        "alone at (inputs, hidden) = (4, 257..320) and (6, 449..512)");
  if (minibatch < 32 || minibatch % 32 || minibatch > MAXK)
    return cfail(VBOC_CLS_EUNSUPPORTED, "minibatch must be a multiple of 32 in [32, 4096]");
  vboc_cls* h = new vboc_cls();
  h->nin = nin;
  h->hidden = hidden;
  h->hp = hp;
  h->bt = minibatch;
  // split of the dW1 rows: about 256 workgroups, each split a multiple of 32 rows
  const int blocks = (hp / 64) * (hp / 64);
  int S = 1;
  while (blocks * S * 2 <= 256 && (minibatch / (S * 2)) % 32 == 0) S *= 2;
  h->S = S;
  with_shape(h, [&](auto sh) {
    using Ly = Lay<decltype(sh)::NIN, decltype(sh)::HP>;
    h->total = Ly::TOTAL;
    h->rec = Ly::REC;
  });
  auto fail_free = [&](hipError_t e, const char* what) {
    vboc_cls_destroy(h);
    return cfail(VBOC_CLS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  hipError_t e;
#define CALLOC(ptr, bytes) \
  if ((e = hipMalloc((void**)&(ptr), (bytes))) != hipSuccess) return fail_free(e, "hipMalloc " #ptr)
  CALLOC(h->P, sizeof(float) * h->total);
  CALLOC(h->M, sizeof(float) * h->total);
  CALLOC(h->V, sizeof(float) * h->total);
  CALLOC(h->Wf, sizeof(float) * hp * hp);
  CALLOC(h->Wb, sizeof(float) * hp * hp);
  CALLOC(h->idx[0], sizeof(int) * minibatch);
  CALLOC(h->idx[1], sizeof(int) * minibatch);
  CALLOC(h->H1p, sizeof(float) * (size_t)hp * minibatch);
  CALLOC(h->dH2p, sizeof(float) * (size_t)hp * minibatch);
  CALLOC(h->part, sizeof(float) * (size_t)(minibatch / R2) * h->rec);
  CALLOC(h->dW1p, sizeof(float) * (size_t)S * hp * hp);
  CALLOC(h->st, sizeof(State));
  CALLOC(h->epart, sizeof(int) * EVG);
  CALLOC(h->etotal, sizeof(long long));
#undef CALLOC
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
  State s{};
  s.seed = seed;
  *h->st_host = s;
  (void)hipMemcpyAsync(h->st, h->st_host, sizeof(State), hipMemcpyHostToDevice, h->stream);
  if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail_free(e, "init");
  *out = h;
  return 0;
}

int vboc_cls_destroy(vboc_cls_handle h) {
  if (!h) return 0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->exec) (void)hipGraphExecDestroy(h->exec);
  void* bufs[] = {h->P, h->M, h->V, h->Wf, h->Wb, h->H1p, h->dH2p, h->part, h->dW1p, h->idx[0], h->idx[1],
                  h->st, h->epart, h->etotal};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (h->st_host) (void)hipHostFree(h->st_host);
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
  if (h->ev_out) (void)hipEventDestroy(h->ev_out);
  if (h->t0) (void)hipEventDestroy(h->t0);
  if (h->t1) (void)hipEventDestroy(h->t1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int vboc_cls_set_params(vboc_cls_handle h, const float* W0, const float* b0, const float* W1, const float* b1,
                        const float* W2, const float* b2, void* stream) {
  if (!h || !W0 || !b0 || !W1 || !b1 || !W2 || !b2) return cfail(VBOC_CLS_EARG, "null argument");
  if (int rc = order(h->ev_in, (hipStream_t)stream, h->stream)) return rc;
  pack(h, const_cast<float*>(W0), const_cast<float*>(b0), const_cast<float*>(W1), const_cast<float*>(b1),
       const_cast<float*>(W2), const_cast<float*>(b2), 0, h->P);
  CCHK(hipGetLastError());
  return order(h->ev_out, h->stream, (hipStream_t)stream);
}

int vboc_cls_get_params(vboc_cls_handle h, int which, float* W0, float* b0, float* W1, float* b1, float* W2,
                        float* b2, void* stream) {
  if (!h || !W0 || !b0 || !W1 || !b1 || !W2 || !b2) return cfail(VBOC_CLS_EARG, "null argument");
  if (which < 0 || which > 2) return cfail(VBOC_CLS_EARG, "which: 0 parameters, 1 exp_avg, 2 exp_avg_sq");
  if (int rc = order(h->ev_in, (hipStream_t)stream, h->stream)) return rc;
  pack(h, W0, b0, W1, b1, W2, b2, 1, which == 0 ? h->P : which == 1 ? h->M : h->V);
  CCHK(hipGetLastError());
  return order(h->ev_out, h->stream, (hipStream_t)stream);
}

int vboc_cls_train(vboc_cls_handle h, const vboc_cls_run_t* r, void* stream) {
  return vboc_cls_train_split(h, r, 0, stream);
}

int vboc_cls_train_split(vboc_cls_handle h, const vboc_cls_run_t* r, long long n_new, void* stream) {
  if (!h || !r || !r->F) return cfail(VBOC_CLS_EARG, "null argument");
  if (r->ld < h->nin + 2) return cfail(VBOC_CLS_EARG, "ld < inputs + 2");
  if (int rc = check_rows(h, r->n, n_new)) return rc;
  if (r->it_max < 1) return cfail(VBOC_CLS_EARG, "it_max < 1");
  // a graph replays an even number of steps, so every replay starts on idx[0]
  const int poll = r->graphs ? (r->poll > 2 ? (r->poll + 1) / 2 * 2 : 2) : (r->poll > 0 ? r->poll : 1);
  Args a;
  memset(&a, 0, sizeof a);
  a.P = h->P; a.M = h->M; a.V = h->V; a.Wf = h->Wf; a.Wb = h->Wb; a.idx = nullptr;
  a.H1p = h->H1p; a.dH2p = h->dH2p; a.part = h->part; a.dW1p = h->dW1p; a.st = h->st;
  a.F = r->F; a.n = r->n; a.n_new = n_new; a.ldF = r->ld; a.Bt = h->bt; a.S = h->S; a.lr = (float)r->lr;
  // loop state of the reference: it = 0, val = 1
  CCHK(hipStreamSynchronize(h->stream));
  State* s = h->st_host;
  CCHK(hipMemcpyAsync(s, h->st, sizeof(State), hipMemcpyDeviceToHost, h->stream));
  CCHK(hipStreamSynchronize(h->stream));
  s->val = r->val0;
  s->stop = r->stop_val;
  s->beta = r->beta;
  s->it = 0;
  s->it_lim = r->it_max;
  s->gate = 1;
  if (int rc = order(h->ev_in, (hipStream_t)stream, h->stream)) return rc;
  CCHK(hipMemcpyAsync(h->st, s, sizeof(State), hipMemcpyHostToDevice, h->stream));
  const unsigned long long d0 = s->draws;
  // the first step's minibatch (draw d0); every later one is drawn beside the step before it
  Args a0 = a;
  a0.idx = h->idx[0];
  hipLaunchKernelGGL(k_sample, dim3(1), dim3(SNT), 0, h->stream, a0);
  CCHK(hipGetLastError());
  const bool same = h->exec && h->key_poll == poll && memcmp(&h->key, &a, sizeof(Args)) == 0;
  if (r->graphs && !same) {
    if (h->exec) {
      (void)hipGraphExecDestroy(h->exec);
      h->exec = nullptr;
    }
    hipGraph_t g;
    CCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    chunk(h, a, poll, 0, h->stream);
    CCHK(hipStreamEndCapture(h->stream, &g));
    hipError_t e = hipGraphInstantiate(&h->exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return cfail(VBOC_CLS_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    h->key = a;
    h->key_poll = poll;
  }
  CCHK(hipEventRecord(h->t0, h->stream));
  long long launched = 0;
  for (;;) {
    if (r->graphs) CCHK(hipGraphLaunch(h->exec, h->stream));
    else chunk(h, a, poll, (int)(launched & 1), h->stream);
    CCHK(hipGetLastError());
    launched += poll;
    CCHK(hipMemcpyAsync(&s->gate, &h->st->gate, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    CCHK(hipStreamSynchronize(h->stream));
    if (!s->gate) break;
    if (launched > r->it_max + poll) return cfail(VBOC_CLS_EHIP, "fit did not stop at it_max");
  }
  CCHK(hipEventRecord(h->t1, h->stream));
  CCHK(hipMemcpyAsync(s, h->st, sizeof(State), hipMemcpyDeviceToHost, h->stream));
  CCHK(hipStreamSynchronize(h->stream));
  // the sampler stream continues after the steps taken (the ones drawn past the stop are dropped), so the next
  // fit draws what a step-by-step loop would
  s->draws = d0 + (unsigned long long)s->it;
  CCHK(hipMemcpyAsync(&h->st->draws, &s->draws, sizeof(s->draws), hipMemcpyHostToDevice, h->stream));
  CCHK(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, h->t0, h->t1);
  if (int rc = order(h->ev_out, h->stream, (hipStream_t)stream)) return rc;
  if (r->iterations) *r->iterations = s->it;
  if (r->val) *r->val = s->val;
  if (r->launched) *r->launched = launched;
  if (r->kernel_ms) *r->kernel_ms = ms;
  return 0;
}

int vboc_cls_sample(vboc_cls_handle h, long long n, int steps, int* idx_out, void* stream) {
  return vboc_cls_sample_split(h, n, 0, steps, idx_out, stream);
}

int vboc_cls_sample_split(vboc_cls_handle h, long long n, long long n_new, int steps, int* idx_out, void* stream) {
  if (!h || !idx_out || steps < 0) return cfail(VBOC_CLS_EARG, "bad argument");
  if (int rc = check_rows(h, n, n_new)) return rc;
  if (int rc = order(h->ev_in, (hipStream_t)stream, h->stream)) return rc;
  Args a;
  memset(&a, 0, sizeof a);
  a.idx = h->idx[0]; a.st = h->st;
  a.n = n; a.n_new = n_new; a.Bt = h->bt; a.S = h->S;
  for (int i = 0; i < steps; ++i) {
    hipLaunchKernelGGL(k_sample, dim3(1), dim3(SNT), 0, h->stream, a);
    CCHK(hipGetLastError());
    CCHK(hipMemcpyAsync(idx_out + (size_t)i * h->bt, h->idx[0], sizeof(int) * h->bt, hipMemcpyDeviceToDevice,
                        h->stream));
  }
  CCHK(hipStreamSynchronize(h->stream));
  return order(h->ev_out, h->stream, (hipStream_t)stream);
}

int vboc_cls_eval(vboc_cls_handle h, const float* X, long long n, int ld, unsigned char* labels, float* logits,
                  long long* count1, void* stream) {
  if (!h) return cfail(VBOC_CLS_EARG, "null handle");
  if (h->hp != HPF) return cfail(VBOC_CLS_EUNSUPPORTED, "a handle with hidden > 128 is a trainer only");
  if (n < 0 || n >= (1ll << 31)) return cfail(VBOC_CLS_EARG, "rows outside [0, 2^31)");
  if (count1) *count1 = 0;
  if (n == 0) return 0;
  if (!X || !labels) return cfail(VBOC_CLS_EARG, "null argument");
  if (ld < h->nin) return cfail(VBOC_CLS_EARG, "ld < inputs");
  EvalArgs e;
  e.P = h->P; e.Wf = h->Wf; e.X = X; e.labels = labels; e.logits = logits; e.part = h->epart; e.n = n; e.ld = ld;
  e.nblk = (int)((n + R2 - 1) / R2);
  const int G = e.nblk < EVG ? e.nblk : EVG;
  if (int rc = order(h->ev_in, (hipStream_t)stream, h->stream)) return rc;
  if (h->nin == 6) hipLaunchKernelGGL((k_eval<6>), dim3(G), dim3(256), 0, h->stream, e);
  else if (h->nin == 4) hipLaunchKernelGGL((k_eval<4>), dim3(G), dim3(256), 0, h->stream, e);
  else hipLaunchKernelGGL((k_eval<2>), dim3(G), dim3(256), 0, h->stream, e);
  hipLaunchKernelGGL(k_count_final, dim3(1), dim3(256), 0, h->stream, h->epart, G, h->etotal);
  CCHK(hipGetLastError());
  long long total = 0;
  CCHK(hipMemcpyAsync(&total, h->etotal, sizeof total, hipMemcpyDeviceToHost, h->stream));
  CCHK(hipStreamSynchronize(h->stream));
  if (count1) *count1 = total;
  return order(h->ev_out, h->stream, (hipStream_t)stream);
}

int vboc_cls_boundary(vboc_cls_handle h, const double* X_test, int m, int nq, float mean, float std, int max_steps,
                      double* err, int* steps, unsigned char* flags, void* stream) {
  if (!h) return cfail(VBOC_CLS_EARG, "null handle");
  if (h->hp != HPF) return cfail(VBOC_CLS_EUNSUPPORTED, "a handle with hidden > 128 is a trainer only");
  if (m < 0) return cfail(VBOC_CLS_EARG, "m < 0");
  if ((nq != 2 && nq != 3) || 2 * nq != h->nin) return cfail(VBOC_CLS_EARG, "the march needs nq 2 or 3 = inputs / 2");
  if (m == 0) return 0;
  if (!X_test || !err || !steps || !flags) return cfail(VBOC_CLS_EARG, "null argument");
  MarchArgs a;
  a.P = h->P; a.Wf = h->Wf; a.X = X_test; a.err = err; a.steps = steps; a.flags = flags;
  a.mean = mean; a.std = std; a.max_steps = max_steps > 0 ? max_steps : MAX_STEPS;
  if (int rc = order(h->ev_in, (hipStream_t)stream, h->stream)) return rc;
  if (nq == 3) hipLaunchKernelGGL((k_boundary<6>), dim3(m), dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL((k_boundary<4>), dim3(m), dim3(256), 0, h->stream, a);
  CCHK(hipGetLastError());
  return order(h->ev_out, h->stream, (hipStream_t)stream);
}

}  // extern "C"
