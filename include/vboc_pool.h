/* vboc_pool.h - C ABI of the pool library of the AL loop (vboc_amd/csrc/pool.hip -> libvboc_pool.so).
 *
 * Replaces, around the AL labelling OCP (plain pointers and sizes, device memory, HIP streams as void*):
 *   AL/triplependulum_al.py:253-264  the entropy of the whole unlabeled pool (sigmoid of the two logits,
 *                                    scipy.stats.entropy), every iteration
 *   AL/triplependulum_al.py:267-281  the B most uncertain rows (np.argpartition, sorted in reverse), their removal
 *                                    from the pool and etpmax
 *   AL/triplependulum_class_al.py:180-192  the guess network's trajectories (compute_problem_nnguess)
 *   AL/triplependulum_al.py:204-227, :396-420  the RMSE march of the held-out states (vboc_pool_boundary)
 *   my_nn.py:4-18                    NeuralNetCLS (Linear-ReLU-Linear-ReLU-Linear)
 * Supported: inputs 2, 4 or 6; hidden 1..512 (padded inside the library to 64, 128, 256, 320 or 512 units, the
 * padded units exactly zero); guess outputs = inputs * N <= 640.  Other shapes return VBOC_POOL_EUNSUPPORTED.
 *
 * Every call queues its kernels on `stream` itself, so it is ordered after the work already queued there; the calls
 * of one handle share scratch buffers and must be issued on one stream at a time.
 */
#ifndef VBOC_POOL_H
#define VBOC_POOL_H

#ifdef __cplusplus
extern "C" {
#endif

#define VBOC_POOL_EARG (-1)
#define VBOC_POOL_EHIP (-2)
#define VBOC_POOL_EUNSUPPORTED (-3)

typedef struct vboc_pool* vboc_pool_handle;

int vboc_pool_create(int inputs, int hidden, vboc_pool_handle* out);
int vboc_pool_destroy(vboc_pool_handle h);

/* Parameters in torch's nn.Linear layouts (device float32): W0 [hidden][inputs], b0 [hidden], W1 [hidden][hidden],
 * b1 [hidden], W2 [2][hidden] (the guess network: [outputs][hidden]), b2. */
int vboc_pool_set_classifier(vboc_pool_handle h, const float* W0, const float* b0, const float* W1, const float* b1,
                             const float* W2, const float* b2, void* stream);
int vboc_pool_set_guess(vboc_pool_handle h, int outputs, const float* W0, const float* b0, const float* W1,
                        const float* b1, const float* W2, const float* b2, void* stream);

/* The classifier over the pool.  X: device float64 [n][inputs] raw states; the input of the network is
 * (float32(x) - mean) / std in float32.  etp (device float32 [n]) = scipy.stats.entropy(sigmoid(logits)) in float32:
 * p = 1 / (1 + exp(-l)), q = p / (p0 + p1), etp = -(q0 log q0 + q1 log q1) with 0 log 0 = 0 and -0 stored as +0; a
 * row whose two sigmoids underflow scores NaN.  logits (device float32 [n][2]) and labels (device uint8 [n], l1 > l0)
 * are optional.  A row's result does not depend on the rows around it.  n = 0 returns without a launch. */
int vboc_pool_entropy(vboc_pool_handle h, const double* X, long long n, float mean, float std, float* etp,
                      float* logits, unsigned char* labels, void* stream);

/* The B rows of largest etp (a radix select; NaN ranks above every number, -0 equals +0; ties at the B-th value go
 * to the lower row index).  idx: device int64 [B], DESCENDING row index.  X ([n][inputs] float64), X_sel
 * ([B][inputs], in idx's order) and X_out (the other n - B rows in their original order; out of place) are optional
 * together.  *etpmax (host, optional) = the largest selected score; NaN when a selected score is NaN.  n = 0 or
 * B = 0 return without a launch (*etpmax = 0); B > n is VBOC_POOL_EARG.  Returns after the stream has drained. */
int vboc_pool_select(vboc_pool_handle h, const float* etp, const double* X, long long n, long long B, int inputs,
                     long long* idx, double* X_sel, double* X_out, float* etpmax, void* stream);

/* The guess network's trajectories: x_guess (device float64 [B][N + 1][inputs]); stage 0 is X0's row itself, stages
 * 1..N the network's output * std + mean (a float32 multiply, then a float32 add) widened to float64.  Needs
 * vboc_pool_set_guess with outputs = inputs * N. */
int vboc_pool_guess(vboc_pool_handle h, const double* X0, long long B, int N, float mean, float std, double* x_guess,
                    void* stream);

/* The RMSE march (AL/triplependulum_al.py:204-227, :396-420; the double's twin) under the handle's classifier.
 * X_test: device float64 [m][inputs] raw states, nq = inputs / 2.  The start label of a ray is l1 > l0 of its row.
 * With vel_norm the float64 norm of the nq velocity components, c_i = (1e-2 v_i) / vel_norm is subtracted (start
 * label 0) or added (start label 1) step by step in float64; point k is the velocity after k such steps, cast to
 * float32, normalised in float32 and classified.  The ray ends at the first point whose label differs from the start
 * label, whose stop norm is not > 1e-2 (a NaN ends it) or whose index is max_steps.  The stop norm is the full norm;
 * with 1 <= outward_dims < nq the rays of start label 1 test the norm of the first outward_dims velocity components
 * instead (the triple's `norm([v0, v1])`).  A ray whose stop norm is not > 1e-2 at the start takes no step.
 * err (device float64 [m]) = vel_norm - the full norm at the stopping point; steps (device int32 [m]) the stopping
 * index; flags (device uint8 [m]): bit 0 the start label, bit 1 "stopped by max_steps alone".  A point's label is
 * exactly what vboc_pool_entropy writes to `labels` for a row holding that point's float32 values; a ray's result does
 * not depend on m or on the other rays.  max_steps <= 0 selects 16384; max_steps > 2^20, m < 0 and outward_dims
 * outside 0..nq are VBOC_POOL_EARG; m = 0 returns without a launch; inputs 2 is VBOC_POOL_EUNSUPPORTED. */
int vboc_pool_boundary(vboc_pool_handle h, const double* X_test, int m, float mean, float std, int max_steps,
                       int outward_dims, double* err, int* steps, unsigned char* flags, void* stream);

const char* vboc_pool_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
