/* vboc_cls.h - C ABI of the classifier library of the HJR (and AL) loops (vboc_amd/csrc/cls.hip -> libvboc_cls.so).
 *
 * Replaces, around the HJR one-step OCP (plain pointers and sizes, device memory, HIP streams as void*):
 *   HJR/triplependulum_hjr.py:95-118, :234-258   NeuralNetCLS / Adam(1e-3) / BCEWithLogitsLoss, the fit
 *                                                (`while val > loss_stop and it < it_max`, random.sample rows)
 *   HJR/triplependulum_hjr.py:136-148, :203-213  the classification of a candidate set (argmax of the two logits)
 *   HJR/triplependulum_hjr.py:150-176            the RMSE march along each held-out state's velocity direction
 *   my_nn.py:4-18                                NeuralNetCLS (Linear-ReLU-Linear-ReLU-Linear, two logits)
 * Supported: inputs 2, 4 or 6, hidden 65..128 (padded to 128), minibatch a multiple of 32 up to 4096 (triple and
 * double 100 / 4096, pendulum 100 / 64).  The fit alone (create, set / get_params, train, sample) also at inputs 4 with
 * hidden 257..320 (padded to 320: the AL double's 300) and inputs 6 with hidden 449..512 (padded to 512: the AL
 * triple's 500); on such a handle vboc_cls_eval and vboc_cls_boundary return VBOC_CLS_EUNSUPPORTED and write nothing
 * (the AL loop classifies and marches through vboc_pool.h).  Other shapes return VBOC_CLS_EUNSUPPORTED.
 */
#ifndef VBOC_CLS_H
#define VBOC_CLS_H

#ifdef __cplusplus
extern "C" {
#endif

#define VBOC_CLS_EARG (-1)
#define VBOC_CLS_EHIP (-2)
#define VBOC_CLS_EUNSUPPORTED (-3)

typedef struct vboc_cls* vboc_cls_handle;

/* A classifier: padded parameters, Adam moments (zero) and step count, the sampler's Philox stream (seed).  The
 * moments and the step count persist across fits, as the reference's one optimizer object does. */
int vboc_cls_create(int inputs, int hidden, int minibatch, unsigned long long seed, vboc_cls_handle* out);
int vboc_cls_destroy(vboc_cls_handle h);

/* Parameters in torch's nn.Linear layouts (device float32): W0 [hidden][inputs], b0 [hidden], W1 [hidden][hidden],
 * b1 [hidden], W2 [2][hidden], b2 [2].  Ordered after the work already queued on `stream`. */
int vboc_cls_set_params(vboc_cls_handle h, const float* W0, const float* b0, const float* W1, const float* b1,
                        const float* W2, const float* b2, void* stream);
/* which: 0 the parameters, 1 Adam's exp_avg, 2 its exp_avg_sq (same layouts) */
int vboc_cls_get_params(vboc_cls_handle h, int which, float* W0, float* b0, float* W1, float* b1, float* W2,
                        float* b2, void* stream);

typedef struct {
  const float* F;        /* device float32 rows [n][ld]: the normalised inputs, then the two targets */
  long long n;           /* rows (>= minibatch) */
  int ld;                /* row stride in floats (>= inputs + 2) */
  long long it_max;      /* the loop runs while val > stop_val and fewer than it_max steps are taken (the pendulum's
                            `it <= it_max` is it_max + 1 here) */
  double val0;           /* the loop's initial val: 1 */
  double stop_val;       /* loss_stop: 5e-3 (pendulum 1e-3) */
  double beta;           /* EMA weight */
  double lr;             /* Adam learning rate 1e-3 */
  int poll;              /* steps per HIP graph / per host poll of the stop flag */
  int graphs;            /* 1: replay a captured graph of `poll` steps; 0: launch the steps one by one */
  long long* iterations; /* out: the steps taken */
  double* val;           /* out: val at the stop */
  long long* launched;   /* out: steps launched (a multiple of poll; the ones past the stop are no-ops) */
  double* kernel_ms;     /* out: device time of the fit on the classifier's stream */
} vboc_cls_run_t;

/* One fit (BCEWithLogitsLoss, mean over 2 x minibatch elements): returns 0 when the loop stopped. */
int vboc_cls_train(vboc_cls_handle h, const vboc_cls_run_t* run, void* stream);

/* `steps` minibatch index draws of the sampler (test hook: the same kernel as the fit; advances the stream) into
 * idx_out (device int32 [steps][minibatch]). */
int vboc_cls_sample(vboc_cls_handle h, long long n, int steps, int* idx_out, void* stream);

/* The same two with a split minibatch (AL/doublependulum_al.py:301-307): with n_new > 0 the last n_new of the n rows
 * are the new ones, and each minibatch is minibatch/2 distinct old rows, then minibatch/2 distinct new rows.
 * n_new = 0 is vboc_cls_train / vboc_cls_sample exactly.  n_new < 0, n_new > n, n_new < minibatch/2 and
 * n - n_new < minibatch/2 (where random.sample would raise) return VBOC_CLS_EARG before anything is queued. */
int vboc_cls_train_split(vboc_cls_handle h, const vboc_cls_run_t* run, long long n_new, void* stream);
int vboc_cls_sample_split(vboc_cls_handle h, long long n, long long n_new, int steps, int* idx_out, void* stream);

/* Forward pass over n device rows X [n][ld] (normalised float32 inputs): labels (device uint8 [n]) = argmax of the
 * two logits (a tie gives 0, as np.argmax), logits (device float32 [n][2], optional), *count1 (host) = the number of
 * rows labelled 1, summed in a fixed order.  n = 0 returns zero. */
int vboc_cls_eval(vboc_cls_handle h, const float* X, long long n, int ld, unsigned char* labels, float* logits,
                  long long* count1, void* stream);

/* The RMSE march (:150-176) for nq = 2 or 3 (inputs = 2 nq): X_test device float64 [m][2 nq] (raw states), mean and
 * std the float32 normalisation scalars.  Per ray: the start label comes from the float32 cast of the row; while
 * the label stays and |v| > 1e-2, v -+= 1e-2 v_test / |v_test| in float64, step by step, and the point is cast to
 * float32, normalised in float32 and classified.  err (device float64 [m]) = |v_test| - |v_final|, steps (device
 * int32 [m]) the steps taken, flags (device uint8 [m]): bit 0 the start label, bit 1 "stopped by max_steps" (the
 * reference's outward march has no bound).  max_steps <= 0 selects 16384. */
int vboc_cls_boundary(vboc_cls_handle h, const double* X_test, int m, int nq, float mean, float std, int max_steps,
                      double* err, int* steps, unsigned char* flags, void* stream);

const char* vboc_cls_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
