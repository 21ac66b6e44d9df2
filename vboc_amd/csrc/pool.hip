// The pool side of the AL loop on the device: the classifier's entropy over the whole unlabeled pool, the selection
// of the B most uncertain rows with the pool's compaction, and the guess network's trajectories.
//
// Reference: AL/triplependulum_al.py:253-264 (sigmoid, scipy.stats.entropy over DataLoader batches), :267-281
// (np.argpartition, the reverse sort, the `del` loop, etpmax), AL/triplependulum_class_al.py:180-192 (the guess
// network around compute_problem_nnguess), my_nn.py:4-18 (NeuralNetCLS), the double's twins.
//
//   k_fwd      64 rows per workgroup and round, hidden padded to HP = 64 NT.  Wave w owns the column tiles w + 4u of
//              H2 = relu(H1 W1' + b1) for all 64 rows (16 NT accumulator registers per row block) on
//              v_mfma_f32_16x16x4_f32; W1 is read as packed fragments straight from L2, once per 64 rows.  H1 is not
//              staged: layer 0 has K <= 6, so each lane recomputes the four H1 values of its A fragment from its
//              rows' inputs and the [W0 | b0] rows kept in LDS.  Epilogue: the two logits and the entropy, or (guess
//              network) H2 to a scratch buffer.
//   k_march    the RMSE march of the held-out states under the classifier (AL/triplependulum_al.py:204-227, :396-420):
//              one ray per workgroup, 64 points per round through k_fwd's tile body (tile_gemm here, out_partials
//              and out_sum in nn_common.h: one copy for both kernels), the start labels from one k_fwd launch.
//   k_out      the guess network's third layer over H2 (16 rows x 256 outputs per workgroup, k-ordered fma chains),
//              out * std + mean, widened to float64 into stages 1..N; stage 0 is x0.
//   selection  a radix select on the scores' bits: four (k_hist, k_pick) passes of 8 bits, then k_count (per-block
//              counts of "above" and "equal to" the threshold), k_scan (one workgroup) and k_scatter.  Integer LDS
//              and global atomics only; kernels never wait for one another except at kernel boundaries.
//
// Every reduction has a fixed order, every loop a bound known at launch; a row's result does not depend on its batch.
// Compiled with -ffp-contract=off: every fma below is written out.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/vboc_pool.h"
#include "nn_common.h"

namespace {

constexpr int RT = 64;          // rows per workgroup and round
constexpr int RB = RT / 16;     // 16-row blocks
constexpr int MAXH = 512;       // largest (padded) hidden size
constexpr int MAXOUT = 640;     // most guess outputs
constexpr int FWG = 2048;       // most workgroups of one forward pass
constexpr int OR = 16;          // rows per workgroup of k_out
constexpr int SB = 2048;        // rows per workgroup of k_count / k_scatter (256 threads x 8)
constexpr int HG = 1024;        // most workgroups of one histogram pass

__host__ __device__ constexpr int stride0(int nin) { return nin == 2 ? 4 : 8; }   // [W0 row | b0 | 0..] in floats

struct FwdArgs {
  const float* W0b;           // [HP][stride0]: W0's row, then b0
  const float* Wf;            // W1 as the product's B fragments: pk(j, k, HP / 16)
  const float* b1;            // [HP]
  const float* W2;            // classifier: [2][HP]
  const float* b2;            // classifier: [2]
  const double* X;            // raw states [n][NIN]
  float* etp;                 // [n]
  float* logits;              // [n][2] or null
  unsigned char* labels;      // [n] or null
  float* H2;                  // [n][HP]: when set, H2 is written and the logit epilogue is skipped
  long long n;
  int ntiles;
  float mean, std;
};

__device__ __forceinline__ float entr(float q) { return q == 0.f ? 0.f : -(q * logf(q)); }

// One k group of 16 of the 64-row tile: the A fragment H1[16 rb + lr][16 t + 4 lq + s] recomputed from the lane's rows
// x and the [W0 | b0] rows in LDS, then MFMA step s sums k = 16 t + 4 lq + s.
template <int NIN, int NT>
__device__ __forceinline__ void tile_group(const float (&x)[RB][NIN], const float* w0s, int t, int lq,
                                           const f4 (&bv)[NT], f4 (&acc)[RB][NT]) {
  constexpr int ST = stride0(NIN);
  const float* wk = w0s + (16 * t + 4 * lq) * ST;
  float av[RB][4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float wc[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) wc[i] = wk[s * ST + i];
    const float bc = wk[s * ST + NIN];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < NIN; ++i) sum = fmaf(x[rb][i], wc[i], sum);
      av[rb][s] = fmaxf(sum + bc, 0.f);
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int u = 0; u < NT; ++u) acc[rb][u] = mfma(av[rb][s], bv[u][s], acc[rb][u]);
}

// The 64-row tile body shared by k_fwd and k_march: acc = H1 W1' for the lane's A rows x[rb] = row 16 rb + lr
// (normalised inputs), wave w's column tiles w + 4u.  Two register sets of B fragments alternate, as in gemm_rows.
// The logits follow through nn_common.h's out_partials / out_sum, so a row's logits are the same bits in both kernels.
template <int NIN, int NT>
__device__ __forceinline__ void tile_gemm(const float (&x)[RB][NIN], const float* w0s, const float* Wf, int w,
                                          int lane, int lq, f4 (&acc)[RB][NT]) {
  constexpr int TG = 4 * NT;      // k groups of 16; even
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int u = 0; u < NT; ++u) acc[rb][u] = f4{0.f, 0.f, 0.f, 0.f};
  const float* bp = Wf + ((size_t)w * TG * 64 + lane) * 4;      // tile u: + u * 4 TG * 256, group t: + 256 t
  f4 b0[NT], b1[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) b0[u] = *(const f4*)(bp + (size_t)u * 4 * TG * 256);
  for (int t = 0; t < TG; t += 2) {
#pragma unroll
    for (int u = 0; u < NT; ++u) b1[u] = *(const f4*)(bp + (size_t)u * 4 * TG * 256 + 256 * (t + 1));
    tile_group<NIN, NT>(x, w0s, t, lq, b0, acc);
    if (t + 2 < TG) {
#pragma unroll
      for (int u = 0; u < NT; ++u) b0[u] = *(const f4*)(bp + (size_t)u * 4 * TG * 256 + 256 * (t + 2));
    }
    tile_group<NIN, NT>(x, w0s, t + 1, lq, b1, acc);
  }
}

template <int NIN, int NT>
__global__ __launch_bounds__(256) void k_fwd(FwdArgs a) {
  constexpr int HP = 64 * NT, ST = stride0(NIN);
  __shared__ __attribute__((aligned(16))) float w0s[HP * ST];
  __shared__ float red[4][RT][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  for (int i = tid; i < HP * ST; i += 256) w0s[i] = a.W0b[i];
  __syncthreads();
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const long long row0 = (long long)tile * RT;
    // this lane's A rows: 16 rb + lr (the last tile's rows are clamped here and masked on output)
    float x[RB][NIN];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      long long row = row0 + 16 * rb + lr;
      row = row < a.n ? row : a.n - 1;
#pragma unroll
      for (int i = 0; i < NIN; ++i) x[rb][i] = ((float)a.X[(size_t)row * NIN + i] - a.mean) / a.std;
    }
    f4 acc[RB][NT];
    tile_gemm<NIN, NT>(x, w0s, a.Wf, w, lane, lq, acc);

    // acc[rb][u][g] = A2[row 16 rb + 4 lq + g][col 16 (w + 4u) + lr]
    if (a.H2) {
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        const int j = 16 * (w + 4 * u) + lr;
        const float bj = a.b1[j];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const long long row = row0 + 16 * rb + 4 * lq + g;
            if (row < a.n) a.H2[(size_t)row * HP + j] = fmaxf(acc[rb][u][g] + bj, 0.f);
          }
      }
      continue;
    }
    out_partials<2, RB, NT>(acc, a.b1, 0, a.W2, 0, HP, w, lr, lq, &red[0][0][0]);
    __syncthreads();
    if (tid < RT && row0 + tid < a.n) {
      const int r = tid;
      const long long row = row0 + r;
      const float l0 = out_sum<2, RB>(&red[0][0][0], r, 0) + a.b2[0];
      const float l1 = out_sum<2, RB>(&red[0][0][0], r, 1) + a.b2[1];
      // scipy.stats.entropy(sigmoid(l)) in float32: pk / sum(pk), then the sum of entr
      const float p0 = 1.f / (1.f + expf(-l0)), p1 = 1.f / (1.f + expf(-l1));
      const float sp = p0 + p1;
      const float e = entr(p0 / sp) + entr(p1 / sp);
      a.etp[row] = e == 0.f ? 0.f : e;        // -0 is stored as +0
      if (a.logits) {
        a.logits[2 * row] = l0;
        a.logits[2 * row + 1] = l1;
      }
      if (a.labels) a.labels[row] = (unsigned char)(l1 > l0);
    }
    __syncthreads();
  }
}

struct MarchArgs {
  const float* W0b;           // the classifier's buffers, as FwdArgs has them
  const float* Wf;
  const float* b1;
  const float* W2;
  const float* b2;
  const double* X;            // held-out states [m][NIN]
  const unsigned char* start; // [m]: k_fwd's labels of X
  double* err;                // [m]
  int* steps;                 // [m]
  unsigned char* flags;       // [m]
  float mean, std;
  int max_steps;
  int od;                     // outward_dims: 0 = the full norm in both directions
};

// The RMSE march (AL/triplependulum_al.py:204-227, :396-420), one ray per workgroup: cls.hip's k_boundary at RT = 64
// points per round under the wide classifier, with the same ray helpers (nn_common.h).  Thread r < RT forms point
// base + r + 1 from the round's base velocity and writes its normalised float32 inputs to the staging tile `xs`; the
// tile body is k_fwd's own (tile_gemm, out_partials) with its A rows read from that tile, so a point's label is what
// k_fwd gives the same float32 row.  The ray's float64 state lives in LDS across the body.  The first point whose label differs from the start label, whose
// stop norm is not > 1e-2 or whose index is max_steps ends the ray; rounds = ceil(max_steps / RT) is known at launch.
template <int NIN, int NT>
__global__ __launch_bounds__(256) void k_march(MarchArgs a) {
  constexpr int HP = 64 * NT, ST = stride0(NIN), NQ = NIN / 2;
  __shared__ __attribute__((aligned(16))) float w0s[HP * ST];
  __shared__ float red[4][RT][2];
  __shared__ float xs[RT][NIN];         // the round's points, normalised
  __shared__ double vb[NQ], vbn[NQ];    // the round's base velocity; point RT's, the next base
  __shared__ double cst[NQ], vn0;       // the step c; vel_norm
  __shared__ double vnl[RT];            // the points' full norms
  __shared__ int stopl[RT];             // bit 0: label differs, bit 1: stop norm not > 1e-2, bit 2: index >= max_steps
  __shared__ int firstl;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int ray = blockIdx.x;
  const double* xr = a.X + (size_t)ray * NIN;
  const int label = a.start[ray];
  const bool partial = label == 1 && a.od >= 1 && a.od < NQ;    // the triple's `norm([v0, v1])` in the outward loop
  {
    double v0[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) v0[i] = xr[NQ + i];
    double sn;
    const double vel_norm = ray_norm<NQ, false>(v0, a.od, partial, sn);
    if (!(sn > 1e-2)) {     // no step taken; every thread of the workgroup sees the same values
      if (tid == 0) {
        a.err[ray] = 0.0;
        a.steps[ray] = 0;
        a.flags[ray] = (unsigned char)label;
      }
      return;
    }
    if (tid < NQ) {
      const double vt = xr[NQ + tid];
      vb[tid] = vt;
      cst[tid] = ray_step(vt, vel_norm, label);
    }
    if (tid == 0) vn0 = vel_norm;
  }
  for (int i = tid; i < HP * ST; i += 256) w0s[i] = a.W0b[i];
  if (tid < RT) {           // the positions do not change along the ray
#pragma unroll
    for (int i = 0; i < NQ; ++i) xs[tid][i] = ((float)xr[i] - a.mean) / a.std;
  }
  __syncthreads();
  const int rounds = (a.max_steps + RT - 1) / RT;
  for (int rd = 0; rd < rounds; ++rd) {
    const int base = rd * RT;
    if (tid < RT) {
      double v[NQ], c[NQ];
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        v[i] = vb[i];
        c[i] = cst[i];
      }
      ray_point<NQ>(v, c, tid);
#pragma unroll
      for (int i = 0; i < NQ; ++i) xs[tid][NQ + i] = ((float)v[i] - a.mean) / a.std;
      double sn;
      vnl[tid] = ray_norm<NQ, false>(v, a.od, partial, sn);
      stopl[tid] = ((!(sn > 1e-2)) << 1) | ((base + tid + 1 >= a.max_steps) << 2);
      if (tid == RT - 1) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) vbn[i] = v[i];
      }
    }
    __syncthreads();

    // k_fwd's tile body over the staging tile (no float64 value is live across it)
    float x[RB][NIN];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int i = 0; i < NIN; ++i) x[rb][i] = xs[16 * rb + lr][i];
    f4 acc[RB][NT];
    tile_gemm<NIN, NT>(x, w0s, a.Wf, w, lane, lq, acc);
    out_partials<2, RB, NT>(acc, a.b1, 0, a.W2, 0, HP, w, lr, lq, &red[0][0][0]);
    __syncthreads();
    // the march's epilogue: wave 0 holds the round's RT points, one per lane
    if (tid < RT) {
      const int r = tid;
      const float l0 = out_sum<2, RB>(&red[0][0][0], r, 0) + a.b2[0];
      const float l1 = out_sum<2, RB>(&red[0][0][0], r, 1) + a.b2[1];
      const int sb = stopl[r] | ((int)(l1 > l0) != label);
      const unsigned long long any = __ballot(sb != 0);
      const int first = any ? __ffsll((long long)any) - 1 : RT;
      if (r == 0) firstl = first;
      if (r == first) {
        a.err[ray] = vn0 - vnl[r];
        a.steps[ray] = base + r + 1;
        a.flags[ray] = (unsigned char)(label | ((sb == 4) << 1));     // bit 1: stopped by max_steps alone
      }
    }
    __syncthreads();
    if (firstl < RT) return;      // uniform: every thread reads the same word after the barrier
    if (tid < NQ) vb[tid] = vbn[tid];
    __syncthreads();
  }
  // not reached: the last round holds index max_steps, whose bit 2 ends the ray
}

// torch layouts -> the padded buffers (H real hidden units; O outputs, OP the padded row length of W2t).  The
// classifier keeps W2 as [2][HP], the guess network as W2t [HP][OP] (transposed: k_out reads it along the outputs).
__global__ void k_pack(const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                       const float* b2, int nin, int H, int HP, int O, int OP, int transposed, float* W0b, float* Wf,
                       float* b1p, float* W2p, float* b2p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int ST = stride0(nin);
  if (i < HP * HP) {
    const int j = i / HP, c = i % HP;
    Wf[pk(j, c, HP / 16)] = (j < H && c < H) ? W1[(size_t)j * H + c] : 0.f;
  }
  if (i < HP * ST) {
    const int c = i / ST, q = i % ST;
    W0b[i] = c < H ? (q < nin ? W0[c * nin + q] : (q == nin ? b0[c] : 0.f)) : 0.f;
  }
  if (i < HP) b1p[i] = i < H ? b1[i] : 0.f;
  if (transposed) {
    if (i < HP * OP) {
      const int k = i / OP, o = i % OP;
      W2p[i] = (k < H && o < O) ? W2[(size_t)o * H + k] : 0.f;
    }
    if (i < OP) b2p[i] = i < O ? b2[i] : 0.f;
  } else {
    if (i < 2 * HP) {
      const int o = i / HP, k = i % HP;
      W2p[i] = k < H ? W2[o * H + k] : 0.f;
    }
    if (i < 2) b2p[i] = b2[i];
  }
}

struct OutArgs {
  const float* H2;            // [B][HP]
  const float* W2t;           // [HP][OP]
  const float* b2;            // [OP]
  const double* X0;           // [B][nin]
  double* xg;                 // [B][N + 1][nin]
  long long B;
  int HP, O, OP, nin;
  float mean, std;
};

// out[b][o] = sum_k H2[b][k] W2[o][k] (k ascending, one fma chain) + b2[o]; then out * std + mean.
__global__ __launch_bounds__(256) void k_out(OutArgs a) {
  __shared__ __attribute__((aligned(16))) float hs[OR * MAXH];
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * OR;
  const int o = blockIdx.y * 256 + tid;
  const int HP = a.HP;
  for (int i = tid; i < OR * HP; i += 256) {
    long long row = row0 + i / HP;
    row = row < a.B ? row : a.B - 1;
    hs[i] = a.H2[(size_t)row * HP + i % HP];
  }
  __syncthreads();
  const size_t stage = (size_t)a.O + a.nin;       // doubles per problem: (N + 1) nin
  if (blockIdx.y == 0 && tid < OR * a.nin) {      // stage 0 is x0 itself
    const long long row = row0 + tid / a.nin;
    if (row < a.B) a.xg[(size_t)row * stage + tid % a.nin] = a.X0[(size_t)row * a.nin + tid % a.nin];
  }
  if (o >= a.O) return;
  float acc[OR];
#pragma unroll
  for (int r = 0; r < OR; ++r) acc[r] = 0.f;
  for (int k = 0; k < HP; k += 4) {
    float wv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) wv[s] = a.W2t[(size_t)(k + s) * a.OP + o];
#pragma unroll
    for (int r = 0; r < OR; ++r) {
      const f4 h = *(const f4*)&hs[r * HP + k];
      acc[r] = fmaf(h.x, wv[0], acc[r]);
      acc[r] = fmaf(h.y, wv[1], acc[r]);
      acc[r] = fmaf(h.z, wv[2], acc[r]);
      acc[r] = fmaf(h.w, wv[3], acc[r]);
    }
  }
  const float bo = a.b2[o];
#pragma unroll
  for (int r = 0; r < OR; ++r) {
    const long long row = row0 + r;
    if (row < a.B) {
      const float v = (acc[r] + bo) * a.std;      // a multiply, then an add: not contracted (-ffp-contract=off)
      a.xg[(size_t)row * stage + a.nin + o] = (double)(v + a.mean);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// selection
// ------------------------------------------------------------------------------------------------
struct SelState {
  unsigned prefix;            // the threshold key's bits found so far
  unsigned maxkey;
  unsigned rem;               // rank still looked for among the keys with this prefix; at the end: the number of
                              // rows equal to the threshold that are selected
  unsigned pad;
  unsigned hist[4][256];
};

// order-preserving key of a score: NaN above +inf, -0 equal to +0
__device__ __forceinline__ unsigned keyof(float v) {
  const unsigned b = __float_as_uint(v);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
  if ((b << 1) == 0u) return 0x80000000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// pass p (0..3): digit (key >> (24 - 8p)) & 255 of the keys whose higher digits equal the prefix
__global__ __launch_bounds__(256) void k_hist(const float* etp, long long n, SelState* st, int p) {
  __shared__ unsigned hs[256];
  const int tid = threadIdx.x;
  hs[tid] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * p;
  const unsigned himask = p == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
  const unsigned prefix = st->prefix;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < n; i += (long long)gridDim.x * 256) {
    const unsigned k = keyof(etp[i]);
    if ((k & himask) == prefix) atomicAdd(&hs[(k >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (hs[tid]) atomicAdd(&st->hist[p][tid], hs[tid]);
}

// one thread: the digit that holds the rem-th largest key of the pass
__global__ void k_pick(SelState* st, int p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned rem = st->rem;
  unsigned cum = 0u;
  int d = 255;
  for (; d > 0; --d) {
    if (cum + st->hist[p][d] >= rem) break;
    cum += st->hist[p][d];
  }
  st->prefix |= (unsigned)d << (24 - 8 * p);
  st->rem = rem - cum;
}

__global__ __launch_bounds__(256) void k_count(const float* etp, long long n, const SelState* st, unsigned* cntA,
                                               unsigned* cntE, SelState* stw) {
  __shared__ unsigned sa[256], se[256], sm[256];
  const int tid = threadIdx.x;
  const unsigned T = st->prefix;
  const long long base = (long long)blockIdx.x * SB + 8 * tid;
  unsigned ca = 0u, ce = 0u, mx = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (base + j < n) {
      const unsigned k = keyof(etp[base + j]);
      ca += k > T;
      ce += k == T;
      mx = k > mx ? k : mx;
    }
  }
  sa[tid] = ca;
  se[tid] = ce;
  sm[tid] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int r = 1; r < 256; ++r) {
      ca += sa[r];
      ce += se[r];
      mx = sm[r] > mx ? sm[r] : mx;
    }
    cntA[blockIdx.x] = ca;
    cntE[blockIdx.x] = ce;
    atomicMax(&stw->maxkey, mx);
  }
}

// exclusive scans of the per-block counts, in place, by one workgroup: thread t owns a contiguous segment
__global__ __launch_bounds__(256) void k_scan(unsigned* cntA, unsigned* cntE, int nblk) {
  __shared__ unsigned sa[256], se[256];
  const int tid = threadIdx.x;
  const int seg = (nblk + 255) / 256;
  const int lo = tid * seg, hi = min(lo + seg, nblk);
  unsigned ca = 0u, ce = 0u;
  for (int i = lo; i < hi; ++i) {
    ca += cntA[i];
    ce += cntE[i];
  }
  sa[tid] = ca;
  se[tid] = ce;
  __syncthreads();
  unsigned oa = 0u, oe = 0u;
  for (int r = 0; r < tid; ++r) {
    oa += sa[r];
    oe += se[r];
  }
  for (int i = lo; i < hi; ++i) {
    const unsigned va = cntA[i], ve = cntE[i];
    cntA[i] = oa;
    cntE[i] = oe;
    oa += va;
    oe += ve;
  }
}

struct ScatArgs {
  const float* etp;
  const double* X;            // or null
  const SelState* st;
  const unsigned* offA;       // scanned counts
  const unsigned* offE;
  long long* idx;
  double* Xsel;
  double* Xout;
  long long n, B;
  int nin;
};

__global__ __launch_bounds__(256) void k_scatter(ScatArgs a) {
  __shared__ unsigned sa[256], se[256];
  const int tid = threadIdx.x;
  const unsigned T = a.st->prefix, need = a.st->rem;
  const long long base = (long long)blockIdx.x * SB + 8 * tid;
  unsigned key[8];
  unsigned ca = 0u, ce = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    key[j] = base + j < a.n ? keyof(a.etp[base + j]) : 0u;
    if (base + j < a.n) {
      ca += key[j] > T;
      ce += key[j] == T;
    }
  }
  sa[tid] = ca;
  se[tid] = ce;
  __syncthreads();
  unsigned ab = a.offA[blockIdx.x], eb = a.offE[blockIdx.x];
  for (int r = 0; r < tid; ++r) {
    ab += sa[r];
    eb += se[r];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long i = base + j;
    if (i >= a.n) break;
    const bool above = key[j] > T, eq = key[j] == T;
    const bool sel = above || (eq && eb < need);
    const long long before = (long long)ab + (eb < need ? eb : need);     // selected rows of lower index
    if (sel) {
      const long long pos = a.B - 1 - before;
      if (pos >= 0 && pos < a.B) {
        a.idx[pos] = i;
        if (a.X)
          for (int c = 0; c < a.nin; ++c) a.Xsel[(size_t)pos * a.nin + c] = a.X[(size_t)i * a.nin + c];
      }
    } else if (a.X) {
      const long long pos = i - before;
      if (pos >= 0 && pos < a.n - a.B)
        for (int c = 0; c < a.nin; ++c) a.Xout[(size_t)pos * a.nin + c] = a.X[(size_t)i * a.nin + c];
    }
    ab += above;
    eb += eq;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct PoolNet {
  float *W0b = nullptr, *Wf = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr;
  int outputs = 0, OP = 0;
  bool set = false;
};

struct vboc_pool {
  int nin, hidden, NT, HP;
  PoolNet cls, gs;
  float* H2 = nullptr;
  size_t H2cap = 0;             // rows
  unsigned *cntA = nullptr, *cntE = nullptr;
  size_t cntcap = 0;
  SelState* st = nullptr;
  unsigned* maxkey_host = nullptr;      // pinned
  float* metp = nullptr;                // the march's start pass: etp [mcap], then the labels [mcap]
  size_t mcap = 0;                      // rays
};

static thread_local std::string g_pool_err;
static int pfail(int code, const std::string& m) {
  g_pool_err = m;
  return code;
}
#define PCHK(x)                                                                          \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) return pfail(VBOC_POOL_EHIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

static int padded_tiles(int hidden) {
  const int nts[] = {1, 2, 4, 5, 8};
  for (int nt : nts)
    if (hidden <= 64 * nt) return nt;
  return 0;
}

static void free_net(PoolNet& p) {
  void* bufs[] = {p.W0b, p.Wf, p.b1, p.W2, p.b2};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  p = PoolNet();
}

static int alloc_net(const vboc_pool* h, PoolNet& p, int w2_floats, int b2_floats) {
  PCHK(hipMalloc((void**)&p.W0b, sizeof(float) * h->HP * stride0(h->nin)));
  PCHK(hipMalloc((void**)&p.Wf, sizeof(float) * (size_t)h->HP * h->HP));
  PCHK(hipMalloc((void**)&p.b1, sizeof(float) * h->HP));
  PCHK(hipMalloc((void**)&p.W2, sizeof(float) * w2_floats));
  PCHK(hipMalloc((void**)&p.b2, sizeof(float) * b2_floats));
  return 0;
}

template <int NIN>
static int launch_fwd_nin(const vboc_pool* h, const FwdArgs& a, int G, hipStream_t s) {
  switch (h->NT) {
    case 1: hipLaunchKernelGGL((k_fwd<NIN, 1>), dim3(G), dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_fwd<NIN, 2>), dim3(G), dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_fwd<NIN, 4>), dim3(G), dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((k_fwd<NIN, 5>), dim3(G), dim3(256), 0, s, a); break;
    case 8: hipLaunchKernelGGL((k_fwd<NIN, 8>), dim3(G), dim3(256), 0, s, a); break;
    default: return pfail(VBOC_POOL_EUNSUPPORTED, "hidden size");
  }
  return 0;
}

static int launch_fwd(const vboc_pool* h, FwdArgs& a, hipStream_t s) {
  const long long tiles = (a.n + RT - 1) / RT;
  a.ntiles = (int)tiles;
  const int G = tiles < FWG ? (int)tiles : FWG;
  int rc;
  if (h->nin == 6) rc = launch_fwd_nin<6>(h, a, G, s);
  else if (h->nin == 4) rc = launch_fwd_nin<4>(h, a, G, s);
  else rc = launch_fwd_nin<2>(h, a, G, s);
  if (rc) return rc;
  PCHK(hipGetLastError());
  return 0;
}

template <int NIN>
static int launch_march_nin(const vboc_pool* h, const MarchArgs& a, int m, hipStream_t s) {
  switch (h->NT) {
    case 1: hipLaunchKernelGGL((k_march<NIN, 1>), dim3(m), dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_march<NIN, 2>), dim3(m), dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_march<NIN, 4>), dim3(m), dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((k_march<NIN, 5>), dim3(m), dim3(256), 0, s, a); break;
    case 8: hipLaunchKernelGGL((k_march<NIN, 8>), dim3(m), dim3(256), 0, s, a); break;
    default: return pfail(VBOC_POOL_EUNSUPPORTED, "hidden size");
  }
  return 0;
}

extern "C" {

const char* vboc_pool_last_error(void) { return g_pool_err.c_str(); }

int vboc_pool_create(int inputs, int hidden, vboc_pool_handle* out) {
  if (!out) return pfail(VBOC_POOL_EARG, "out is null");
  *out = nullptr;
  if ((inputs != 2 && inputs != 4 && inputs != 6) || hidden < 1 || hidden > MAXH)
    return pfail(VBOC_POOL_EUNSUPPORTED, "the pool library supports inputs 2, 4, 6 and hidden 1..512");
  vboc_pool* h = new vboc_pool();
  h->nin = inputs;
  h->hidden = hidden;
  h->NT = padded_tiles(hidden);
  h->HP = 64 * h->NT;
  hipError_t e;
  if ((e = hipMalloc((void**)&h->st, sizeof(SelState))) != hipSuccess ||
      (e = hipHostMalloc((void**)&h->maxkey_host, sizeof(unsigned))) != hipSuccess) {
    vboc_pool_destroy(h);
    return pfail(VBOC_POOL_EHIP, std::string("allocation: ") + hipGetErrorString(e));
  }
  *out = h;
  return 0;
}

int vboc_pool_destroy(vboc_pool_handle h) {
  if (!h) return 0;
  (void)hipDeviceSynchronize();
  free_net(h->cls);
  free_net(h->gs);
  void* bufs[] = {h->H2, h->cntA, h->cntE, h->st, h->metp};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (h->maxkey_host) (void)hipHostFree(h->maxkey_host);
  delete h;
  return 0;
}

int vboc_pool_set_classifier(vboc_pool_handle h, const float* W0, const float* b0, const float* W1, const float* b1,
                             const float* W2, const float* b2, void* stream) {
  if (!h || !W0 || !b0 || !W1 || !b1 || !W2 || !b2) return pfail(VBOC_POOL_EARG, "null argument");
  if (!h->cls.W0b) {
    if (int rc = alloc_net(h, h->cls, 2 * h->HP, 2)) {
      free_net(h->cls);
      return rc;
    }
  }
  PoolNet& p = h->cls;
  p.outputs = 2;
  const int total = h->HP * h->HP;
  hipLaunchKernelGGL(k_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, W0, b0, W1, b1, W2, b2,
                     h->nin, h->hidden, h->HP, 2, 0, 0, p.W0b, p.Wf, p.b1, p.W2, p.b2);
  PCHK(hipGetLastError());
  p.set = true;
  return 0;
}

int vboc_pool_set_guess(vboc_pool_handle h, int outputs, const float* W0, const float* b0, const float* W1,
                        const float* b1, const float* W2, const float* b2, void* stream) {
  if (!h || !W0 || !b0 || !W1 || !b1 || !W2 || !b2) return pfail(VBOC_POOL_EARG, "null argument");
  if (outputs < h->nin || outputs > MAXOUT || outputs % h->nin)
    return pfail(VBOC_POOL_EUNSUPPORTED, "guess outputs must be inputs * N, at most 640");
  const int OP = (outputs + 63) / 64 * 64;
  if (h->gs.W0b && h->gs.OP != OP) {
    PCHK(hipDeviceSynchronize());
    free_net(h->gs);
  }
  if (!h->gs.W0b) {
    if (int rc = alloc_net(h, h->gs, h->HP * OP, OP)) {
      free_net(h->gs);
      return rc;
    }
  }
  PoolNet& p = h->gs;
  p.outputs = outputs;
  p.OP = OP;
  int total = h->HP * h->HP;
  if (h->HP * OP > total) total = h->HP * OP;
  hipLaunchKernelGGL(k_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, W0, b0, W1, b1, W2, b2,
                     h->nin, h->hidden, h->HP, outputs, OP, 1, p.W0b, p.Wf, p.b1, p.W2, p.b2);
  PCHK(hipGetLastError());
  p.set = true;
  return 0;
}

int vboc_pool_entropy(vboc_pool_handle h, const double* X, long long n, float mean, float std, float* etp,
                      float* logits, unsigned char* labels, void* stream) {
  if (!h) return pfail(VBOC_POOL_EARG, "null handle");
  if (n < 0 || n >= (1ll << 31)) return pfail(VBOC_POOL_EARG, "rows outside [0, 2^31)");
  if (n == 0) return 0;
  if (!X || !etp) return pfail(VBOC_POOL_EARG, "null argument");
  if (!h->cls.set) return pfail(VBOC_POOL_EARG, "vboc_pool_set_classifier has not been called");
  FwdArgs a;
  memset(&a, 0, sizeof a);
  a.W0b = h->cls.W0b; a.Wf = h->cls.Wf; a.b1 = h->cls.b1; a.W2 = h->cls.W2; a.b2 = h->cls.b2;
  a.X = X; a.etp = etp; a.logits = logits; a.labels = labels; a.H2 = nullptr; a.n = n; a.mean = mean; a.std = std;
  return launch_fwd(h, a, (hipStream_t)stream);
}

int vboc_pool_boundary(vboc_pool_handle h, const double* X_test, int m, float mean, float std, int max_steps,
                       int outward_dims, double* err, int* steps, unsigned char* flags, void* stream) {
  if (!h) return pfail(VBOC_POOL_EARG, "null handle");
  if (h->nin == 2) return pfail(VBOC_POOL_EUNSUPPORTED, "the march takes inputs 4 and 6");
  if (m < 0) return pfail(VBOC_POOL_EARG, "m < 0");
  if (outward_dims < 0 || outward_dims > h->nin / 2) return pfail(VBOC_POOL_EARG, "outward_dims outside 0..nq");
  if (max_steps > (1 << 20)) return pfail(VBOC_POOL_EARG, "max_steps > 2^20");
  if (max_steps <= 0) max_steps = 16384;
  if (m == 0) return 0;
  if (!X_test || !err || !steps || !flags) return pfail(VBOC_POOL_EARG, "null argument");
  if (!h->cls.set) return pfail(VBOC_POOL_EARG, "vboc_pool_set_classifier has not been called");
  hipStream_t s = (hipStream_t)stream;
  if ((size_t)m > h->mcap) {
    PCHK(hipStreamSynchronize(s));
    if (h->metp) (void)hipFree(h->metp);
    h->metp = nullptr;
    h->mcap = 0;
    PCHK(hipMalloc((void**)&h->metp, (sizeof(float) + 1) * (size_t)m));
    h->mcap = (size_t)m;
  }
  unsigned char* start = (unsigned char*)(h->metp + h->mcap);
  // the start labels: one forward pass over X_test itself
  FwdArgs f;
  memset(&f, 0, sizeof f);
  f.W0b = h->cls.W0b; f.Wf = h->cls.Wf; f.b1 = h->cls.b1; f.W2 = h->cls.W2; f.b2 = h->cls.b2;
  f.X = X_test; f.etp = h->metp; f.logits = nullptr; f.labels = start; f.H2 = nullptr; f.n = m; f.mean = mean;
  f.std = std;
  if (int rc = launch_fwd(h, f, s)) return rc;
  MarchArgs a;
  a.W0b = f.W0b; a.Wf = f.Wf; a.b1 = f.b1; a.W2 = f.W2; a.b2 = f.b2;
  a.X = X_test; a.start = start; a.err = err; a.steps = steps; a.flags = flags; a.mean = mean; a.std = std;
  a.max_steps = max_steps; a.od = outward_dims == h->nin / 2 ? 0 : outward_dims;
  int rc = h->nin == 6 ? launch_march_nin<6>(h, a, m, s) : launch_march_nin<4>(h, a, m, s);
  if (rc) return rc;
  PCHK(hipGetLastError());
  return 0;
}

int vboc_pool_select(vboc_pool_handle h, const float* etp, const double* X, long long n, long long B, int inputs,
                     long long* idx, double* X_sel, double* X_out, float* etpmax, void* stream) {
  if (!h) return pfail(VBOC_POOL_EARG, "null handle");
  if (n < 0 || n >= (1ll << 31) || B < 0) return pfail(VBOC_POOL_EARG, "rows outside [0, 2^31)");
  if (B > n) return pfail(VBOC_POOL_EARG, "B > n (the caller clamps B to the pool's remainder)");
  if (etpmax) *etpmax = 0.f;
  if (n == 0 || B == 0) return 0;
  if (!etp || !idx) return pfail(VBOC_POOL_EARG, "null argument");
  if (X && (!X_sel || (!X_out && B < n))) return pfail(VBOC_POOL_EARG, "X needs X_sel and X_out");
  if (X && inputs < 1) return pfail(VBOC_POOL_EARG, "inputs < 1");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = (int)((n + SB - 1) / SB);
  if ((size_t)nblk > h->cntcap) {
    PCHK(hipStreamSynchronize(s));
    if (h->cntA) (void)hipFree(h->cntA);
    if (h->cntE) (void)hipFree(h->cntE);
    h->cntA = h->cntE = nullptr;
    h->cntcap = 0;
    PCHK(hipMalloc((void**)&h->cntA, sizeof(unsigned) * nblk));
    PCHK(hipMalloc((void**)&h->cntE, sizeof(unsigned) * nblk));
    h->cntcap = nblk;
  }
  PCHK(hipMemsetAsync(h->st, 0, sizeof(SelState), s));
  const unsigned rem0 = (unsigned)B;
  PCHK(hipMemcpyAsync(&h->st->rem, &rem0, sizeof rem0, hipMemcpyHostToDevice, s));
  const long long hb = (n + 255) / 256;
  const int HGn = hb < HG ? (int)hb : HG;
  for (int p = 0; p < 4; ++p) {
    hipLaunchKernelGGL(k_hist, dim3(HGn), dim3(256), 0, s, etp, n, h->st, p);
    hipLaunchKernelGGL(k_pick, dim3(1), dim3(64), 0, s, h->st, p);
  }
  hipLaunchKernelGGL(k_count, dim3(nblk), dim3(256), 0, s, etp, n, h->st, h->cntA, h->cntE, h->st);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(256), 0, s, h->cntA, h->cntE, nblk);
  ScatArgs a;
  a.etp = etp; a.X = X; a.st = h->st; a.offA = h->cntA; a.offE = h->cntE; a.idx = idx; a.Xsel = X_sel;
  a.Xout = X_out; a.n = n; a.B = B; a.nin = inputs;
  hipLaunchKernelGGL(k_scatter, dim3(nblk), dim3(256), 0, s, a);
  PCHK(hipGetLastError());
  PCHK(hipMemcpyAsync(h->maxkey_host, &h->st->maxkey, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  PCHK(hipStreamSynchronize(s));
  if (etpmax) {
    const unsigned k = *h->maxkey_host;
    const unsigned b = k == 0xFFFFFFFFu ? 0x7FC00000u : ((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
    memcpy(etpmax, &b, sizeof b);
  }
  return 0;
}

int vboc_pool_guess(vboc_pool_handle h, const double* X0, long long B, int N, float mean, float std, double* x_guess,
                    void* stream) {
  if (!h) return pfail(VBOC_POOL_EARG, "null handle");
  if (B < 0 || B >= (1ll << 31)) return pfail(VBOC_POOL_EARG, "rows outside [0, 2^31)");
  if (!h->gs.set) return pfail(VBOC_POOL_EARG, "vboc_pool_set_guess has not been called");
  if (N < 1 || N * h->nin != h->gs.outputs) return pfail(VBOC_POOL_EARG, "N * inputs differs from the guess outputs");
  if (B == 0) return 0;
  if (!X0 || !x_guess) return pfail(VBOC_POOL_EARG, "null argument");
  hipStream_t s = (hipStream_t)stream;
  if ((size_t)B > h->H2cap) {
    PCHK(hipStreamSynchronize(s));
    if (h->H2) (void)hipFree(h->H2);
    h->H2 = nullptr;
    h->H2cap = 0;
    PCHK(hipMalloc((void**)&h->H2, sizeof(float) * (size_t)B * h->HP));
    h->H2cap = (size_t)B;
  }
  FwdArgs a;
  memset(&a, 0, sizeof a);
  a.W0b = h->gs.W0b; a.Wf = h->gs.Wf; a.b1 = h->gs.b1; a.W2 = nullptr; a.b2 = nullptr;
  a.X = X0; a.H2 = h->H2; a.n = B; a.mean = mean; a.std = std;
  if (int rc = launch_fwd(h, a, s)) return rc;
  OutArgs o;
  o.H2 = h->H2; o.W2t = h->gs.W2; o.b2 = h->gs.b2; o.X0 = X0; o.xg = x_guess; o.B = B; o.HP = h->HP;
  o.O = h->gs.outputs; o.OP = h->gs.OP; o.nin = h->nin; o.mean = mean; o.std = std;
  hipLaunchKernelGGL(k_out, dim3((unsigned)((B + OR - 1) / OR), (unsigned)((o.O + 255) / 256)), dim3(256), 0, s, o);
  PCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
