"""Boundary-velocity regressor of VBOC: the NN fit on the generated boundary states and its RMSE on
the held-out set.

Reference: my_nn.py:20-34 (NeuralNetDIR), VBOC/triplependulum_vboc.py:407-491 (first fit + RMSE),
:493-566 (refits as data arrives), the double VBOC/doublependulum_vboc.py:440-560 and the pendulum
VBOC/pendulum_vboc.py:35-41,228-292.

Model input = [ (q - mean) / std , qdot / |qdot| ], target = |qdot|  (:55-65); mean/std are the
scalar mean and (unbiased) std over ALL position entries, computed in float32 as the reference does
with torch.tensor(X[:, :nq].tolist()) (:50).  Training: Adam(lr 1e-3) on MSE, minibatch 4096 drawn
without replacement, EMA of the loss `val = 0.95 val + 0.05 loss` starting at max|qdot|; stop when
val <= 1e-3 or after it_max = 10 * int(n_0 * 100 / 4096) steps (:67-99), n_0 = size of the first
dataset (B and it_max are fixed once, :68-69).  Refits sample half of each minibatch from the old
rows and half from the new ones (:156-166).

MI355X design (the NN stays PyTorch-ROCm): the reference rebuilds each minibatch on
the host from Python lists (:164-165) and syncs on loss.item() every step.  Here the feature matrix
lives in HBM as float32, minibatch indices are drawn on the device (a uniform random k-subset = the
top-k of n uniform keys), and one training step - sampling, forward, backward, Adam, the EMA and the
stop test - is captured once in a HIP graph and replayed.  The stop test is evaluated on the device
and gates the update (a step taken after the stop condition is a no-op), so the host only polls the
`active` flag every `poll` steps while the iteration count and the final model are exactly those of
the reference's per-step loop.
"""
import math

import numpy as np
import torch
import torch.nn as nn


# ------------------------------------------------------------------------------------------------
# models (my_nn.py): same module structure, so state_dicts load in the reference's scripts
# ------------------------------------------------------------------------------------------------
class NeuralNetDIR(nn.Module):
    """my_nn.py:20-34: Linear-ReLU-Linear-ReLU-Linear-ReLU (non-negative output = |qdot|)."""

    def __init__(self, input_size, hidden_size, output_size):
        super().__init__()
        self.linear_relu_stack = nn.Sequential(
            nn.Linear(input_size, hidden_size), nn.ReLU(),
            nn.Linear(hidden_size, hidden_size), nn.ReLU(),
            nn.Linear(hidden_size, output_size), nn.ReLU())

    def forward(self, x):
        return self.linear_relu_stack(x)


class NeuralNetCLS(nn.Module):
    """my_nn.py:4-18 (the AL / HJR classifiers' architecture; loaded by the comparison scripts)."""

    def __init__(self, input_size, hidden_size, output_size):
        super().__init__()
        self.linear_relu_stack = nn.Sequential(
            nn.Linear(input_size, hidden_size), nn.ReLU(),
            nn.Linear(hidden_size, hidden_size), nn.ReLU(),
            nn.Linear(hidden_size, output_size))

    def forward(self, x):
        return self.linear_relu_stack(x)


# layer sizes per system: triple 6-500-1 (:38-41), double 4-300-1 (doublependulum_vboc.py:448-451),
# pendulum 2-100-1 (pendulum_vboc.py:35-37), minibatch 4096 / 4096 / 64
HIDDEN = {3: 500, 2: 300, 1: 100}
MINIBATCH = {3: 4096, 2: 4096, 1: 64}


# ------------------------------------------------------------------------------------------------
# data transforms
# ------------------------------------------------------------------------------------------------
def position_stats(X, nq):
    """(mean, std) of all position entries X[:, :nq], in float32 like
    torch.mean(torch.tensor(X[:, :nq].tolist())) (:50); returned as Python floats."""
    t = torch.from_numpy(np.ascontiguousarray(X[:, :nq], dtype=np.float64)).to(torch.float32)
    return torch.mean(t).item(), torch.std(t).item()


def dir_features(X, mean, std, nq):
    """[n, 2nq+1] float64: normalised positions, velocity direction (0 if qdot = 0), |qdot|
    (:55-65).  |qdot| is the sequential sum of squares; the reference's per-row numpy.linalg.norm
    can differ in the last bit of the float64 value, never after the cast to float32 the model sees."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((X.shape[0], 2 * nq + 1))
    out[:, :nq] = (X[:, :nq] - mean) / std
    V = X[:, nq:2 * nq]
    s = V[:, 0] * V[:, 0]
    for j in range(1, nq):
        s = s + V[:, j] * V[:, j]
    vn = np.sqrt(s)
    nz = vn != 0
    out[nz, nq:2 * nq] = V[nz] / vn[nz, None]
    out[:, 2 * nq] = vn
    return out


# ------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------
class DirTrainer:
    """Adam/MSE fit of NeuralNetDIR with the reference's stop rule, device-resident.

    fit(F, n_new) trains on the feature matrix F ([n, 2nq+1], float) - the whole set for the first
    fit (:77-99), or old rows F[:n-n_new] and new rows F[n-n_new:] half-and-half for a refit
    (:156-184)."""

    def __init__(self, nq, device="cpu", hidden=None, minibatch=None, lr=1e-3, beta=0.95, stop_val=1e-3,
                 seed=0, graphs=None, poll=64, it_max=None):
        self.nq = nq
        self.nin = 2 * nq
        self.device = torch.device(device)
        torch.manual_seed(seed)
        self.hidden = hidden or HIDDEN[nq]
        self.model = NeuralNetDIR(self.nin, self.hidden, 1).to(self.device)
        self.k = minibatch or MINIBATCH[nq]
        self.lr, self.beta, self.stop_val = lr, beta, stop_val
        self.b1, self.b2, self.eps = 0.9, 0.999, 1e-8       # torch.optim.Adam defaults (:44)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        self.params = [p for p in self.model.parameters()]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.step_t = torch.zeros((), device=self.device)   # Adam step count (device-side)
        self.graphs = (self.device.type == "cuda") if graphs is None else graphs
        self.poll = poll
        self.it_max = it_max      # None: set by the first fit from its dataset (:68-69)
        self.total_steps = 0
        self.seed, self.fits = seed, 0
        # Every buffer a captured step writes or reads across fits is allocated ONCE, here, outside any capture:
        # the gradients (backward accumulates into them after an in-graph zero_(), instead of allocating them in
        # the graph's private pool, where a new capture would find the previous graph's blocks), and the stop
        # rule's state (val, it, it_lim, active: refilled per fit, never re-allocated).  See fit() for the sampler.
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.val = torch.zeros((), device=self.device)
        self.it = torch.ones((), dtype=torch.int64, device=self.device)
        self.it_lim = torch.zeros((), dtype=torch.int64, device=self.device)
        self.active = torch.ones((), dtype=torch.bool, device=self.device)

    # -- one gated step, written with device tensors only (capturable) ---------------------------------
    # top-k slices are kept at most this long: a uniform k-subset of a long range is the top-k of the per-chunk
    # top-k candidates (exactly the same index set as one top-k over all keys).  A refit of the triple's VBOC loop
    # at configs[2]'s scale faulted the GPU (illegal address, profiles/r03f_vboc_loop_fault.log) in the first fit
    # whose halves exceeded 2^20 rows; the fits before it (halves of 0.5M rows) had run in the same process.
    TOPK_CHUNK = 1 << 18

    def _sample(self, lo, hi, k, gen=None):
        n = hi - lo
        keys = torch.rand(n, device=self.device, generator=gen or self.gen)
        if n <= self.TOPK_CHUNK:
            return torch.topk(keys, k, sorted=False).indices + lo
        c = self.TOPK_CHUNK
        m = (n + c - 1) // c
        pad = torch.full((m * c - n,), -1.0, device=self.device)        # keys are in [0, 1): pads never win
        part = torch.topk(torch.cat([keys, pad]).view(m, c), k, dim=1, sorted=False)
        cand = part.indices + (torch.arange(m, device=self.device) * c).unsqueeze(1)
        best = torch.topk(part.values.reshape(-1), k, sorted=False).indices
        return cand.reshape(-1).index_select(0, best) + lo

    def _step(self, F, X, y, n, n_new, gen=None):
        if n_new:
            idx = torch.cat([self._sample(0, n - n_new, self.k // 2, gen), self._sample(n - n_new, n, self.k // 2, gen)])
        else:
            idx = self._sample(0, n, self.k, gen)
        xb = X.index_select(0, idx)
        yb = y.index_select(0, idx)
        active = (self.val > self.stop_val) & (self.it < self.it_lim)
        a = active.to(torch.float32)
        for p in self.params:
            p.grad.zero_()
        loss = torch.mean((self.model(xb) - yb) ** 2)
        loss.backward()
        grads = [p.grad for p in self.params]
        with torch.no_grad():
            # Adam, torch.optim.Adam's arithmetic (single-tensor path), every update scaled by the gate
            self.step_t.add_(a)
            w1 = a * (1 - self.b1)
            w2 = a * (1 - self.b2)
            for m, v, g in zip(self.m, self.v, grads):
                m.lerp_(g, w1)
                v.mul_(1 - w2).addcmul_(g * w2, g)
            t = torch.clamp(self.step_t, min=1.0)
            bc1 = 1 - torch.pow(self.b1, t)
            bc2s = torch.sqrt(1 - torch.pow(self.b2, t))
            step = -(a * self.lr) / bc1
            for p, m, v in zip(self.params, self.m, self.v):
                p.addcdiv_(m * step, v.sqrt().div_(bc2s).add_(self.eps))
            # the reference's EMA and counter (:95-96), gated as well
            self.val.copy_(torch.where(active, self.beta * self.val + (1 - self.beta) * loss.detach(), self.val))
            self.it.add_(active.to(self.it.dtype))
            self.active.copy_(active)

    def fit(self, F, n_new=0, it_max=None):
        """Train until val <= stop_val or it_max steps.  Returns dict(iterations, val)."""
        F = torch.as_tensor(np.asarray(F), dtype=torch.float32).to(self.device) if not torch.is_tensor(F) \
            else F.to(self.device, torch.float32)
        n = F.shape[0]
        if self.it_max is None:
            B = int(n * 100 / self.k)   # :68, from the first dataset only
            self.it_max = B * 10
        it_max = it_max or self.it_max
        if n_new and (n_new < self.k // 2 or n - n_new < self.k // 2):
            raise ValueError("a refit needs at least minibatch/2 old and new rows")
        if not n_new and n < self.k:
            raise ValueError(f"need at least {self.k} rows (random.sample of a minibatch)")
        X = F[:, :self.nin].contiguous()
        y = F[:, self.nin:self.nin + 1].contiguous()
        self.val.copy_(torch.max(F[:, self.nin]))          # :73 val = max |qdot|
        self.it.fill_(1)
        self.it_lim.fill_(it_max)
        self.active.fill_(True)
        self.fits += 1
        steps = 0
        # Each fit draws from a generator of its own, seeded from the trainer's seed and the fit's index, in both
        # modes (so a captured fit equals the eager one).  A captured fit's graph is the only one that registers
        # it: re-registering one generator with a second graph after the first was destroyed is the pattern that
        # ran in the round-3 fault (profiles/r03f_vboc_loop_fault.log), and nothing of a
        # destroyed graph is referenced by the next one.
        gen = torch.Generator(device=self.device)
        gen.manual_seed(self.fit_seed(self.seed, self.fits))
        if self.graphs:
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):                      # warm-up outside capture (allocations)
                self._step(F, X, y, n, n_new, gen)
            torch.cuda.current_stream(self.device).wait_stream(s)
            steps += 1
            g = torch.cuda.CUDAGraph()
            g.register_generator_state(gen)                  # replays advance this fit's Philox offset
            with torch.cuda.graph(g):
                self._step(F, X, y, n, n_new, gen)
            while bool(self.active.item()):
                for _ in range(self.poll):
                    g.replay()
                steps += self.poll
            torch.cuda.synchronize(self.device)
            del g
        else:
            while bool(self.active.item()):
                self._step(F, X, y, n, n_new, gen)
                steps += 1
        self.total_steps += steps
        return dict(iterations=int(self.it.item()) - 1, val=float(self.val.item()), launched=steps)

    @staticmethod
    def fit_seed(seed, fit):
        """The seed of the minibatch generator of a trainer's fit number `fit` (1, 2, ...)."""
        return seed * 1_000_003 + fit

    @torch.no_grad()
    def predict(self, Xin, batch=1 << 15):
        """Model output for [n, 2nq] inputs in minibatches of 2^15 (VBOC/vboc.py:532-541)."""
        X = torch.as_tensor(np.asarray(Xin), dtype=torch.float32).to(self.device) if not torch.is_tensor(Xin) \
            else Xin.to(self.device, torch.float32)
        return torch.cat([self.model(X[i:i + batch]) for i in range(0, X.shape[0], batch)]) if X.shape[0] else \
            torch.zeros((0, 1), device=self.device)

    @torch.no_grad()
    def rmse(self, F):
        """sqrt(MSELoss(model(F[:, :2nq]), F[:, 2nq:])) (:117-120)."""
        F = torch.as_tensor(np.asarray(F), dtype=torch.float32).to(self.device) if not torch.is_tensor(F) \
            else F.to(self.device, torch.float32)
        out = self.predict(F[:, :self.nin])
        return math.sqrt(torch.mean((out - F[:, self.nin:self.nin + 1]) ** 2).item())

    # -- pruning and the safety margin (VBOC/vboc.py:564-642) ------------------------------------------
    def _prune_targets(self):
        """(module, name) in the reference's tuple order: the three weights, then the three biases (:566-573)."""
        st = self.model.linear_relu_stack
        return [(st[i], name) for name in ("weight", "bias") for i in (0, 2, 4)]

    def n_params(self):
        return sum(p.numel() for p in self.model.parameters())

    def prune(self, amount=0.5):
        """prune.global_unstructured(L1Unstructured, amount) over the six tensors (:575-579): the round(amount * n)
        entries of smallest magnitude are masked.  The `*_orig` parameters are the Parameter objects the trainer
        already holds (self.params, their .grad buffers, Adam's moments), and the step reaches the masks through
        the modules' forward pre-hooks, so the next fit() is the reference's refit under the masks (:592-616) with
        the same optimizer.  Returns the number of entries pruned."""
        import torch.nn.utils.prune as tprune
        tprune.global_unstructured(self._prune_targets(), pruning_method=tprune.L1Unstructured, amount=amount)
        return int(sum(int((m == 0).sum()) for m in self.masks()))

    def prune_remove(self):
        """prune.remove on the six tensors (:620-625): the masks go, the zeros stay, and a later fit trains every
        parameter again.  Adam's moments keep their positions."""
        import torch.nn.utils.prune as tprune
        for mod, name in self._prune_targets():
            if hasattr(mod, name + "_mask"):
                tprune.remove(mod, name)
        self.params = [p for p in self.model.parameters()]
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)

    def masks(self):
        """The six 0 / 1 masks in parameter order (W0, b0, W1, b1, W2, b2); all ones when nothing is pruned."""
        st = self.model.linear_relu_stack
        out = []
        for i in (0, 2, 4):
            for name in ("weight", "bias"):
                m = getattr(st[i], name + "_mask", None)
                ref = getattr(st[i], name)
                out.append(m.detach().clone() if m is not None else torch.ones_like(ref))
        return out

    def safety_margin(self, F):
        """max (out_i - y_i) / y_i over the rows of F ([n, 2nq+1] features) with out_i > y_i (VBOC/vboc.py:638-642):
        out is the float32 model output, the ratio is formed in float64 from the target as given (float64 for a
        float64 array).  A fraction; Safe MPC's `safety_margin` option is a percentage, 100 times this.  The
        reference raises when no output exceeds its target (np.amax of an empty array); here that case is 0.0."""
        if torch.is_tensor(F):
            y = F[:, self.nin].detach().cpu().double().numpy()
        else:
            y = np.asarray(F)[:, self.nin].astype(np.float64)
        X = F[:, :self.nin] if torch.is_tensor(F) else np.asarray(F)[:, :self.nin]
        out = self.predict(X).reshape(-1).cpu().double().numpy()
        d = out - y
        over = d > 0
        return float(np.max(d[over] / y[over])) if over.any() else 0.0


class HipTrainer(DirTrainer):
    """DirTrainer's fit on the device kernels of csrc/fit.hip (libvboc_fit.so, include/vboc_fit.h): sampling,
    forward, backward, Adam and the stop rule of VBOC/triplependulum_vboc.py:446-466 / :526-556 in four kernels
    per step, `poll` steps per HIP graph.  The torch module stays the source of truth between fits (its
    parameters are packed into the trainer before a fit and written back after it); Adam's moments and step count
    live in the trainer across fits, as the reference's one optimizer does.  Differences from DirTrainer: the
    minibatch draws (Philox, random.sample's redraw-on-repeat set method, instead of the top-k of uniform keys)
    and val, kept in float64 as the reference's Python float."""

    def __init__(self, nq, device="cuda", hidden=None, minibatch=None, lr=1e-3, beta=0.95, stop_val=1e-3, seed=0,
                 graphs=True, poll=64, it_max=None):
        import ctypes
        from . import fitlib
        super().__init__(nq, device, hidden=hidden, minibatch=minibatch, lr=lr, beta=beta, stop_val=stop_val,
                         seed=seed, graphs=False, poll=poll, it_max=it_max)
        if self.device.type != "cuda":
            raise ValueError("HipTrainer runs on a GPU (use DirTrainer on the CPU)")
        self._fl = fitlib
        self._lib = fitlib.load()
        h = ctypes.c_void_p()
        fitlib.check(self._lib.vboc_fit_create(self.nin, self.hidden, self.k, seed, ctypes.byref(h)))
        self._h = h
        self.use_graphs = graphs
        self.last = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.vboc_fit_destroy(h)
            self._h = None

    def _param_ptrs(self):
        st = self.model.linear_relu_stack
        ps = [st[0].weight, st[0].bias, st[2].weight, st[2].bias, st[4].weight, st[4].bias]
        for p in ps:
            if not p.is_contiguous() or p.dtype != torch.float32 or not p.is_cuda:
                raise ValueError("model parameters must be contiguous float32 tensors on the trainer's device")
        return [p.data_ptr() for p in ps]

    def fit(self, F, n_new=0, it_max=None):
        import ctypes
        fl = self._fl
        if torch.is_tensor(F):
            Ft = F.to(self.device, torch.float32).contiguous()
            val0 = float(Ft[:, self.nin].max())
        else:
            Fn = np.asarray(F)
            val0 = float(np.max(Fn[:, self.nin]))          # :446, over the float64 features
            Ft = torch.as_tensor(Fn, dtype=torch.float32).to(self.device).contiguous()
        n = Ft.shape[0]
        if self.it_max is None:
            self.it_max = int(n * 100 / self.k) * 10
        it_max = it_max or self.it_max
        if n_new and (n_new < self.k // 2 or n - n_new < self.k // 2):
            raise ValueError("a refit needs at least minibatch/2 old and new rows")
        if not n_new and n < self.k:
            raise ValueError(f"need at least {self.k} rows (random.sample of a minibatch)")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ptrs = self._param_ptrs()
        fl.check(self._lib.vboc_fit_set_params(self._h, *ptrs, stream))
        its, val, launched, ms = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        run = fl.FitRun(F=Ft.data_ptr(), n=n, n_new=n_new, ld=Ft.shape[1], it_max=it_max, val0=val0,
                        stop_val=self.stop_val, beta=self.beta, lr=self.lr, poll=self.poll,
                        graphs=int(self.use_graphs), iterations=ctypes.addressof(its), val=ctypes.addressof(val),
                        launched=ctypes.addressof(launched), kernel_ms=ctypes.addressof(ms))
        fl.check(self._lib.vboc_fit_train(self._h, ctypes.byref(run), stream))
        fl.check(self._lib.vboc_fit_get_params(self._h, 0, *ptrs, stream))
        self.total_steps += launched.value
        self.last = dict(iterations=its.value, val=val.value, launched=launched.value, fit_ms=ms.value)
        return dict(iterations=its.value, val=val.value, launched=launched.value)

    # -- pruning: the mask lives in the native trainer, the torch module stays plain ----------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def prune(self, amount=0.5):
        """DirTrainer.prune on the device (vboc_fit_prune): the round(amount * n) entries of smallest magnitude
        (Python's round, as torch's) are selected by a radix select over the packed parameters, masked and zeroed;
        the zeros are written back to the module.  Ties at the threshold magnitude go in the order W0, b0, b1, W2,
        b2, W1, row-major in each (torch's own tie choice is unspecified).  Until prune_remove() every fit masks
        the gradient and holds the pruned entries at zero.  Returns the number of entries pruned."""
        import ctypes
        k = round(amount * self.n_params())
        ptrs = self._param_ptrs()
        self._fl.check(self._lib.vboc_fit_set_params(self._h, *ptrs, self._stream()))
        got = ctypes.c_longlong()
        self._fl.check(self._lib.vboc_fit_prune(self._h, k, ctypes.byref(got), self._stream()))
        self._fl.check(self._lib.vboc_fit_get_params(self._h, 0, *ptrs, self._stream()))
        return got.value

    def set_mask(self, masks=None):
        """Make the six 0 / 1 tensors (parameter order) the mask, or remove the mask (None).  The module's masked
        entries are zeroed as the trainer's are."""
        ptrs = self._param_ptrs()
        if masks is None:
            self._fl.check(self._lib.vboc_fit_set_mask(self._h, *([None] * 6), self._stream()))
            return
        ms = [m.to(self.device, torch.float32).contiguous() for m in masks]
        if [tuple(m.shape) for m in ms] != [tuple(p.shape) for p in self.model.parameters()]:
            raise ValueError("masks must have the parameters' shapes")
        self._fl.check(self._lib.vboc_fit_set_params(self._h, *ptrs, self._stream()))
        self._fl.check(self._lib.vboc_fit_set_mask(self._h, *[m.data_ptr() for m in ms], self._stream()))
        self._fl.check(self._lib.vboc_fit_get_params(self._h, 0, *ptrs, self._stream()))
        torch.cuda.current_stream(self.device).synchronize()     # `ms` must outlive the copy

    def prune_remove(self):
        self.set_mask(None)

    def masks(self):
        ts = [torch.empty_like(p) for p in self.model.parameters()]
        self._fl.check(self._lib.vboc_fit_get_mask(self._h, *[t.data_ptr() for t in ts], self._stream()))
        return ts

    def evaluate(self, F):
        """Forward-only pass of the module's current parameters over the feature rows F ([n, 2nq+1]) on the device
        kernel (vboc_fit_eval, the training forward's arithmetic): dict(rmse, safety_margin, over, out) with
        rmse = sqrt(mean (out - y)^2) accumulated in float64, the safety margin of DirTrainer.safety_margin, the
        count of rows with out > y, and out the [n, 1] float32 outputs.  The target is the float64 column when F is
        a float64 array, else the float32 one promoted.  Fixed-order reductions: repeated calls return the same
        bits."""
        import ctypes
        y = None
        if torch.is_tensor(F):
            Ft = F.to(self.device, torch.float32).contiguous()
            if F.dtype == torch.float64:
                y = F[:, self.nin].to(self.device).contiguous()
        else:
            Fn = np.asarray(F)
            Ft = torch.as_tensor(Fn, dtype=torch.float32).to(self.device).contiguous()
            if Fn.dtype == np.float64:
                y = torch.as_tensor(np.ascontiguousarray(Fn[:, self.nin])).to(self.device)
        n = Ft.shape[0]
        out = torch.empty((n, 1), dtype=torch.float32, device=self.device)
        stats = (ctypes.c_double * 3)()
        self._fl.check(self._lib.vboc_fit_set_params(self._h, *self._param_ptrs(), self._stream()))
        ptr = lambda t: t.data_ptr() if (t is not None and n) else None
        self._fl.check(self._lib.vboc_fit_eval(self._h, ptr(Ft), n, Ft.shape[1], ptr(y), ptr(out), stats,
                                               self._stream()))
        return dict(rmse=math.sqrt(stats[0] / n) if n else 0.0, safety_margin=stats[1], over=int(stats[2]), out=out)

    def safety_margin(self, F):
        return self.evaluate(F)["safety_margin"]

    def moments(self):
        """Adam's (exp_avg, exp_avg_sq) as lists of tensors in the model's parameter order (test hook)."""
        out = []
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for which in (1, 2):
            ts = [torch.empty_like(p) for p in self.model.parameters()]
            self._fl.check(self._lib.vboc_fit_get_params(self._h, which, *[t.data_ptr() for t in ts], stream))
            out.append(ts)
        return out

    def sample(self, n, n_new=0, steps=1):
        """The sampler's next `steps` minibatches ([steps, k] int32 row indices; test hook)."""
        out = torch.empty((steps, self.k), dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._fl.check(self._lib.vboc_fit_sample(self._h, n, n_new, steps, out.data_ptr(), stream))
        return out


def make_trainer(nq, device="cpu", native=False, **kw):
    """The fit of the VBOC loop: DirTrainer - PyTorch-ROCm, the reference's my_nn.py loop
    (VBOC/triplependulum_vboc.py:409-468) as north_star asks - by default.  native=True selects the native device
    trainer (HipTrainer, csrc/fit.hip) on a GPU for the shapes it implements (triple 6-500, double / Cartesian 4-300,
    pendulum 2-100, minibatch <= 4096; tests/test_fit_device.py pins it to torch Adam); other shapes and the CPU keep
    DirTrainer."""
    from . import fitlib
    dev = torch.device(device)
    hidden = kw.get("hidden") or HIDDEN.get(nq, 0)
    k = kw.get("minibatch") or MINIBATCH.get(nq, 0)
    if native and dev.type == "cuda" and fitlib.supported(2 * nq, hidden, k):
        return HipTrainer(nq, device, **kw)
    return DirTrainer(nq, device, **kw)


# ------------------------------------------------------------------------------------------------
# the HJR / AL classifier (HJR/triplependulum_hjr.py:95-176): BCE fit, classification, RMSE march
# ------------------------------------------------------------------------------------------------
CLS_MINIBATCH = {3: 4096, 2: 4096, 1: 64}       # n_minibatch of the three HJR drivers
CLS_MAX_STEPS = 16384                           # bound of the outward march (the reference has none)


def march_reference(classify, X_test, mean, std, max_steps=CLS_MAX_STEPS, outward_dims=None):
    """The march of HJR/triplependulum_hjr.py:150-176 restated over all rays at once.  `classify(P)` returns the
    labels of the float32 rows P [r, 2nq] (raw states; the normalisation (P - mean) / std is the caller's, inside
    classify).  Every ray accumulates its velocity step by step in float64, as the reference does; one call of
    classify serves step k of every ray still marching.  Returns (err, steps, flags) as vboc_cls_boundary does.
    outward_dims: the outward loop (start label 1) tests the norm of the first `outward_dims` velocity components
    only, as the triple's AL march does (`norm([v0, v1])`, AL/triplependulum_al.py:221, :413); the inward loop and
    the error keep the full norm.  None: the full norm in both loops."""
    X = np.asarray(X_test, dtype=np.float64)
    m, nq = X.shape[0], X.shape[1] // 2
    vt = X[:, nq:]
    s2 = vt[:, 0] * vt[:, 0]
    for j in range(1, nq):
        s2 = s2 + vt[:, j] * vt[:, j]
    vel_norm = np.sqrt(s2)
    label = np.asarray(classify(X.astype(np.float32))).astype(np.int64)
    if outward_dims is not None:
        return _march_outward_dims(classify, X, vel_norm, label, max_steps, outward_dims)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(label[:, None] == 1, -1.0, 1.0) * ((1e-2 * vt) / vel_norm[:, None])
    v = vt.copy()
    vn = vel_norm.copy()
    steps = np.zeros(m, dtype=np.int32)
    capped = np.zeros(m, dtype=bool)
    act = np.flatnonzero(vel_norm > 1e-2)
    while act.size:
        v[act] = v[act] - c[act]
        steps[act] += 1
        q2 = v[act, 0] * v[act, 0]
        for j in range(1, nq):
            q2 = q2 + v[act, j] * v[act, j]
        vn[act] = np.sqrt(q2)
        out = np.asarray(classify(np.c_[X[act, :nq], v[act]].astype(np.float32))).astype(np.int64)
        go = (out == label[act]) & (vn[act] > 1e-2)
        cap = go & (steps[act] >= max_steps)
        capped[act[cap]] = True
        act = act[go & ~cap]
    flags = (label | (capped.astype(np.int64) << 1)).astype(np.uint8)
    return vel_norm - vn, steps, flags


def _march_outward_dims(classify, X, vel_norm, label, max_steps, d):
    """march_reference with the outward loop's stop test on the first d velocity components."""
    m, nq = X.shape[0], X.shape[1] // 2
    vt = X[:, nq:]

    def norms(V):
        full = V[:, 0] * V[:, 0]
        for j in range(1, nq):
            full = full + V[:, j] * V[:, j]
        part = V[:, 0] * V[:, 0]
        for j in range(1, d):
            part = part + V[:, j] * V[:, j]
        return np.sqrt(full), np.sqrt(part)

    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(label[:, None] == 1, -1.0, 1.0) * ((1e-2 * vt) / vel_norm[:, None])
    v = vt.copy()
    vn = vel_norm.copy()
    steps = np.zeros(m, dtype=np.int32)
    capped = np.zeros(m, dtype=bool)
    act = np.flatnonzero(np.where(label == 1, norms(vt)[1], vel_norm) > 1e-2)
    while act.size:
        v[act] = v[act] - c[act]
        steps[act] += 1
        full, part = norms(v[act])
        vn[act] = full
        out = np.asarray(classify(np.c_[X[act, :nq], v[act]].astype(np.float32))).astype(np.int64)
        go = (out == label[act]) & (np.where(label[act] == 1, part, full) > 1e-2)
        cap = go & (steps[act] >= max_steps)
        capped[act[cap]] = True
        act = act[go & ~cap]
    flags = (label | (capped.astype(np.int64) << 1)).astype(np.uint8)
    return vel_norm - vn, steps, flags


class ClsTrainer:
    """The reference's classifier loop on PyTorch: NeuralNetCLS(2nq, hidden, 2), BCEWithLogitsLoss, Adam(lr), one
    optimizer for the whole run; fit() is `while val > loss_stop and it < it_max` with val from 1
    (HJR/triplependulum_hjr.py:95-118).  The CPU path and the comparator of HipClsTrainer.

    fit(F, it_max): F [n, 2nq + 2] float32 = normalised inputs, then the two targets.  The minibatch rows come from
    `self.sampler(n, 1)`: by default random.sample of a random.Random(seed), or an injected callable (n, steps) ->
    [steps, k] indices.  predict_labels / boundary_errors run on the device kernels (libvboc_cls.so) when the model
    is on a GPU and the shape is `clslib.supported` (they are not the NN fit), else on PyTorch.  The native handle
    exists for every `clslib.fit_supported` shape; at hidden > 128 it is a trainer only (HipClsTrainer's)."""

    def __init__(self, nq, device="cpu", hidden=100, minibatch=None, lr=1e-3, beta=0.95, stop_val=5e-3, seed=0,
                 sampler=None, native_eval=True, max_steps=CLS_MAX_STEPS):
        import random
        self.nq, self.nin = nq, 2 * nq
        self.device = torch.device(device)
        torch.manual_seed(seed)
        self.hidden = hidden
        self.model = NeuralNetCLS(self.nin, hidden, 2).to(self.device)
        self.k = minibatch or CLS_MINIBATCH[nq]
        self.lr, self.beta, self.stop_val, self.seed = lr, beta, stop_val, seed
        self.opt = torch.optim.Adam(self.model.parameters(), lr=lr)
        self.crit = nn.BCEWithLogitsLoss()
        self._rng = random.Random(seed)
        self.sampler = sampler or self.sample
        self.max_steps = max_steps
        self.total_steps = 0
        self.last = None
        self._h = None
        self._cl = None
        self._fwd = False           # the handle also classifies and marches (hidden <= 128)
        if native_eval and self.device.type == "cuda":
            from . import clslib
            if clslib.fit_supported(self.nin, hidden, self.k):  # a missing library is an error, not a fall-back
                import ctypes
                self._cl, self._lib = clslib, clslib.load()
                h = ctypes.c_void_p()
                clslib.check(self._lib.vboc_cls_create(self.nin, hidden, self.k, seed, ctypes.byref(h)))
                self._h = h
                self._fwd = clslib.supported(self.nin, hidden, self.k)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.vboc_cls_destroy(h)
            self._h = None

    def sample(self, n, steps=1):
        """The next `steps` minibatches, [steps, k] row indices: random.sample(range(n), k) each."""
        return np.array([self._rng.sample(range(n), self.k) for _ in range(steps)], dtype=np.int64)

    def _rows(self, F):
        return torch.as_tensor(np.asarray(F), dtype=torch.float32).to(self.device).contiguous() \
            if not torch.is_tensor(F) else F.to(self.device, torch.float32).contiguous()

    def fit(self, F, it_max):
        F = self._rows(F)
        n = F.shape[0]
        if n < self.k:
            raise ValueError(f"need at least {self.k} rows (random.sample of a minibatch)")
        it, val = 0, 1.0
        while val > self.stop_val and it < it_max:
            idx = torch.as_tensor(np.asarray(self.sampler(n, 1)).reshape(-1), dtype=torch.long, device=self.device)
            loss = self.crit(self.model(F[idx, :self.nin]), F[idx, self.nin:self.nin + 2])
            loss.backward()
            self.opt.step()
            self.opt.zero_grad()
            val = self.beta * val + (1 - self.beta) * loss.item()
            it += 1
        self.total_steps += it
        self.last = dict(iterations=it, val=val, launched=it)
        return dict(self.last)

    # -- the forward pass: device kernels on a GPU, PyTorch otherwise ----------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _param_ptrs(self):
        ps = list(self.model.parameters())
        for p in ps:
            if not p.is_contiguous() or p.dtype != torch.float32 or not p.is_cuda:
                raise ValueError("model parameters must be contiguous float32 tensors on the trainer's device")
        return [p.data_ptr() for p in ps]

    def _push(self):
        self._cl.check(self._lib.vboc_cls_set_params(self._h, *self._param_ptrs(), self._stream()))

    @torch.no_grad()
    def predict_labels(self, X, batch=1 << 15, logits=False):
        """(labels uint8 [n] on the trainer's device, count of label 1) for the normalised float32 rows X [n, 2nq]:
        argmax of the two logits, a tie gives 0 (:136-148).  logits=True appends the [n, 2] logits."""
        X = self._rows(X)
        n = X.shape[0]
        if self._fwd:
            import ctypes
            lab = torch.empty((n,), dtype=torch.uint8, device=self.device)
            lg = torch.empty((n, 2), dtype=torch.float32, device=self.device) if logits else None
            cnt = ctypes.c_longlong()
            self._push()
            self._cl.check(self._lib.vboc_cls_eval(self._h, X.data_ptr() if n else None, n, X.shape[1] if n else 0,
                                                   lab.data_ptr() if n else None,
                                                   lg.data_ptr() if (logits and n) else None, ctypes.byref(cnt),
                                                   self._stream()))
            return (lab, int(cnt.value), lg) if logits else (lab, int(cnt.value))
        out = torch.cat([self.model(X[i:i + batch]) for i in range(0, n, batch)]) if n else \
            torch.zeros((0, 2), device=self.device)
        lab = (out[:, 1] > out[:, 0]).to(torch.uint8)
        return (lab, int(lab.sum().item()), out) if logits else (lab, int(lab.sum().item()))

    @torch.no_grad()
    def boundary_errors(self, X_test, mean, std, max_steps=None):
        """The RMSE march (:150-176) of every held-out state: dict(err [m] float64, steps, flags, capped, rmse)."""
        max_steps = max_steps or self.max_steps
        X = np.ascontiguousarray(X_test, dtype=np.float64)
        m = X.shape[0]
        mean_t = torch.as_tensor(mean, dtype=torch.float32).to(self.device)
        std_t = torch.as_tensor(std, dtype=torch.float32).to(self.device)
        if self._fwd and self.nq in (2, 3):
            Xd = torch.as_tensor(X).to(self.device)
            err = torch.empty((m,), dtype=torch.float64, device=self.device)
            steps = torch.empty((m,), dtype=torch.int32, device=self.device)
            flags = torch.empty((m,), dtype=torch.uint8, device=self.device)
            self._push()
            if m:
                self._cl.check(self._lib.vboc_cls_boundary(self._h, Xd.data_ptr(), m, self.nq, float(mean_t),
                                                           float(std_t), max_steps, err.data_ptr(), steps.data_ptr(),
                                                           flags.data_ptr(), self._stream()))
            err, steps, flags = err.cpu().numpy(), steps.cpu().numpy(), flags.cpu().numpy()
        else:
            def classify(P):
                out = self.model((torch.from_numpy(P).to(self.device) - mean_t) / std_t)
                return (out[:, 1] > out[:, 0]).cpu().numpy()
            err, steps, flags = march_reference(classify, X, mean, std, max_steps)
        rmse = math.sqrt(np.sum(np.power(err, 2)) / m) if m else 0.0
        return dict(err=err, steps=steps, flags=flags, capped=int(((flags >> 1) & 1).sum()), rmse=rmse)


class HipClsTrainer(ClsTrainer):
    """ClsTrainer's fit on the device kernels of csrc/cls.hip (libvboc_cls.so, include/vboc_cls.h): sampling,
    forward, BCE, backward, Adam and the stop rule in three kernels per step, `poll` steps per HIP graph.  The torch
    module stays the source of truth between fits; Adam's moments and step count live in the native trainer across
    fits.  The minibatches are the native sampler's (Philox, random.sample's set method); `sample` advances it.
    n_new > 0 (fit and sample) draws half of each minibatch from the first n - n_new rows and half from the last n_new
    (AL/doublependulum_al.py:301-307).  Shapes: clslib.fit_supported; at hidden > 128 predict_labels and
    boundary_errors stay on PyTorch."""

    def __init__(self, nq, device="cuda", graphs=True, poll=64, **kw):
        super().__init__(nq, device, native_eval=True, **kw)
        if self._h is None:
            raise ValueError("HipClsTrainer needs a GPU, libvboc_cls.so and a supported shape")
        self.use_graphs, self.poll = graphs, poll

    def sample(self, n, steps=1, n_new=0):
        out = torch.empty((steps, self.k), dtype=torch.int32, device=self.device)
        self._cl.check(self._lib.vboc_cls_sample_split(self._h, n, n_new, steps, out.data_ptr(), self._stream()))
        return out.cpu().numpy().astype(np.int64)

    def fit(self, F, it_max, n_new=0):
        import ctypes
        F = self._rows(F)
        n = F.shape[0]
        if n < self.k:
            raise ValueError(f"need at least {self.k} rows (random.sample of a minibatch)")
        ptrs = self._param_ptrs()
        self._push()
        its, val, launched, ms = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        run = self._cl.ClsRun(F=F.data_ptr(), n=n, ld=F.shape[1], it_max=it_max, val0=1.0, stop_val=self.stop_val,
                              beta=self.beta, lr=self.lr, poll=self.poll, graphs=int(self.use_graphs),
                              iterations=ctypes.addressof(its), val=ctypes.addressof(val),
                              launched=ctypes.addressof(launched), kernel_ms=ctypes.addressof(ms))
        self._cl.check(self._lib.vboc_cls_train_split(self._h, ctypes.byref(run), n_new, self._stream()))
        self._cl.check(self._lib.vboc_cls_get_params(self._h, 0, *ptrs, self._stream()))
        self.total_steps += launched.value
        self.last = dict(iterations=its.value, val=val.value, launched=launched.value, fit_ms=ms.value)
        return dict(iterations=its.value, val=val.value, launched=launched.value)

    def moments(self):
        """Adam's (exp_avg, exp_avg_sq) as lists of tensors in the model's parameter order (test hook)."""
        out = []
        for which in (1, 2):
            ts = [torch.empty_like(p) for p in self.model.parameters()]
            self._cl.check(self._lib.vboc_cls_get_params(self._h, which, *[t.data_ptr() for t in ts], self._stream()))
            out.append(ts)
        return out


def make_cls_trainer(nq, device="cpu", native=False, **kw):
    """The classifier of the HJR loop: ClsTrainer (PyTorch) by default; native=True selects HipClsTrainer on a GPU
    for the shapes csrc/cls.hip trains (clslib.fit_supported; make_trainer's rule).  Either way a GPU run at
    hidden <= 128 classifies and marches on the device kernels."""
    from . import clslib
    dev = torch.device(device)
    if native and dev.type == "cuda" and clslib.fit_supported(2 * nq, kw.get("hidden", 100),
                                                              kw.get("minibatch") or CLS_MINIBATCH[nq]):
        return HipClsTrainer(nq, device, **kw)
    return ClsTrainer(nq, device, **kw)


# ------------------------------------------------------------------------------------------------
# the AL loop's pool side (AL/triplependulum_al.py:253-281) and its guess network (:172-200, :353-387)
# ------------------------------------------------------------------------------------------------
POOL_BATCH = 1 << 15            # n_minibatch_model of the AL drivers


class PoolScorer:
    """The unlabeled pool's entropy, the top-B selection, the guess trajectories and the RMSE march of the AL loop.

    On a GPU (native=True, the default there) the four run on csrc/pool.hip (libvboc_pool.so, include/vboc_pool.h):
    the pool is a float64 device tensor, scored, selected from and compacted without visiting the host, and the
    guesses come out in the layout Solver.al_solve_device(x_guess=...) takes.  native=False is the reference's own
    arithmetic on PyTorch / NumPy (the CPU path and the comparator): DataLoader batches of 2^15 through the module,
    scipy.stats.entropy, np.argpartition(etp, -B)[-B:] sorted in reverse, al.nn_guess per state; the pool is a
    NumPy array.  The parameters are pushed from the two torch modules at every call."""

    def __init__(self, nq, cls_model, guess_model=None, device="cpu", native=None):
        self.nq, self.nin = nq, 2 * nq
        self.device = torch.device(device)
        self.cls_model, self.guess_model = cls_model, guess_model
        self.native = (self.device.type == "cuda") if native is None else bool(native)
        self.calls = dict(entropy=[], select=[], guess=[], boundary=[])     # seconds per call (synchronised)
        self._h = None
        if self.native:
            import ctypes
            from . import poollib
            if self.device.type != "cuda":
                raise ValueError("the native PoolScorer runs on a GPU")
            hidden = cls_model.linear_relu_stack[0].out_features
            if not poollib.supported(self.nin, hidden):
                raise ValueError(f"libvboc_pool.so does not implement inputs {self.nin}, hidden {hidden}")
            self._pl, self._lib = poollib, poollib.load()       # a missing library is an error, not a fall-back
            h = ctypes.c_void_p()
            poollib.check(self._lib.vboc_pool_create(self.nin, hidden, ctypes.byref(h)))
            self._h = h
            self.hidden = hidden

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.vboc_pool_destroy(h)
            self._h = None

    # -- helpers --------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ptrs(self, model):
        ps = list(model.parameters())
        for p in ps:
            if not p.is_contiguous() or p.dtype != torch.float32 or not p.is_cuda:
                raise ValueError("model parameters must be contiguous float32 tensors on the scorer's device")
        return [p.data_ptr() for p in ps]

    def _timed(self, key, fn):
        import time
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        t = time.perf_counter()
        out = fn()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.calls[key].append(time.perf_counter() - t)
        return out

    def _dev_rows(self, t, dtype, cols, what):
        """The native calls take raw pointers: a tensor of another dtype, device or layout would be read out of
        bounds, so it is refused here."""
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or \
                (t.dim() != 1 if cols is None else (t.dim() != 2 or t.shape[1] != cols)):
            shape = "[n]" if cols is None else f"[n, {cols}]"
            raise ValueError(f"{what} must be a contiguous {dtype} cuda tensor {shape} (see to_pool)")
        return t

    def to_pool(self, X):
        """The pool in the scorer's own form: a float64 device tensor (native) or a float64 NumPy array."""
        if self.native:
            if torch.is_tensor(X):
                return X.to(self.device, torch.float64).contiguous()
            return torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64)).to(self.device)
        return X.detach().cpu().double().numpy() if torch.is_tensor(X) else np.ascontiguousarray(X, dtype=np.float64)

    # -- the entropy of every pool row (:253-264) -----------------------------------------------------
    @torch.no_grad()
    def entropy(self, X, mean, std, logits=False):
        """etp of the rows of X [n, 2nq] (raw states): a float32 device tensor (native) or the reference's float64
        array of float32 values.  logits=True returns (etp, logits [n, 2])."""
        return self._timed("entropy", lambda: self._entropy(X, mean, std, logits))

    def _entropy(self, X, mean, std, logits):
        n = X.shape[0]
        if self.native:
            X = self._dev_rows(X, torch.float64, self.nin, "the pool")
            etp = torch.empty((n,), dtype=torch.float32, device=self.device)
            lg = torch.empty((n, 2), dtype=torch.float32, device=self.device) if logits else None
            if n:
                self._pl.check(self._lib.vboc_pool_set_classifier(self._h, *self._ptrs(self.cls_model), self._stream()))
                self._pl.check(self._lib.vboc_pool_entropy(self._h, X.data_ptr(), n, float(mean), float(std),
                                                           etp.data_ptr(), lg.data_ptr() if logits else None, None,
                                                           self._stream()))
            return (etp, lg) if logits else etp
        from scipy.stats import entropy
        from torch.utils.data import DataLoader
        sigmoid = nn.Sigmoid()
        etp = np.empty((n,))
        lgs = []
        mean_t = torch.as_tensor(mean, dtype=torch.float32).to(self.device)
        std_t = torch.as_tensor(std, dtype=torch.float32).to(self.device)
        if n:
            Xt = torch.from_numpy(np.asarray(X, dtype=np.float32)).to(self.device)
            Xt = (Xt - mean_t) / std_t
            for idx, batch in enumerate(DataLoader(Xt, batch_size=POOL_BATCH, shuffle=False)):
                out = self.cls_model(batch)
                prob_xu = sigmoid(out).cpu()
                etp[POOL_BATCH * idx:min(POOL_BATCH * (idx + 1), n)] = entropy(prob_xu, axis=1)
                if logits:
                    lgs.append(out.cpu())
        if logits:
            return etp, (torch.cat(lgs) if lgs else torch.zeros((0, 2)))
        return etp

    # -- the RMSE march of the held-out states (:204-227, :396-420) -----------------------------------
    @torch.no_grad()
    def boundary(self, X_test, mean, std, max_steps=None, outward_dims=None):
        """ClsTrainer.boundary_errors' dict (err [m] float64, steps, flags, capped, rmse) for the raw states X_test
        [m, 2nq] under the classifier.  outward_dims: march_reference's (the triple's AL march passes 2).  Native: one
        vboc_pool_boundary call, every point labelled by the library's own forward pass; else march_reference on the
        module."""
        return self._timed("boundary", lambda: self._boundary(X_test, mean, std, max_steps or CLS_MAX_STEPS,
                                                              outward_dims or None))

    def _boundary(self, X_test, mean, std, max_steps, outward_dims):
        X = self.to_pool(X_test)
        m = X.shape[0]
        if self.native:
            X = self._dev_rows(X, torch.float64, self.nin, "X_test")
            err = torch.empty((m,), dtype=torch.float64, device=self.device)
            steps = torch.empty((m,), dtype=torch.int32, device=self.device)
            flags = torch.empty((m,), dtype=torch.uint8, device=self.device)
            if m:
                self._pl.check(self._lib.vboc_pool_set_classifier(self._h, *self._ptrs(self.cls_model), self._stream()))
                self._pl.check(self._lib.vboc_pool_boundary(self._h, X.data_ptr(), m, float(mean), float(std),
                                                            max_steps, outward_dims or 0, err.data_ptr(),
                                                            steps.data_ptr(), flags.data_ptr(), self._stream()))
            err, steps, flags = err.cpu().numpy(), steps.cpu().numpy(), flags.cpu().numpy()
        else:
            mean_t = torch.as_tensor(mean, dtype=torch.float32).to(self.device)
            std_t = torch.as_tensor(std, dtype=torch.float32).to(self.device)

            def classify(P):
                out = self.cls_model((torch.from_numpy(P).to(self.device) - mean_t) / std_t)
                return (out[:, 1] > out[:, 0]).cpu().numpy()
            err, steps, flags = march_reference(classify, X, mean, std, max_steps, outward_dims)
        rmse = math.sqrt(np.sum(np.power(err, 2)) / m) if m else 0.0
        return dict(err=err, steps=steps, flags=flags, capped=int(((flags >> 1) & 1).sum()), rmse=rmse)

    # -- the B most uncertain rows and the pool without them (:267-281) -------------------------------
    def select(self, etp, X, B):
        """dict(idx [B] int64 NumPy, descending row index; scores [B] (etp[idx], NumPy); X_sel [B, 2nq] the rows in
        that order; X_rest the other rows in their order; etpmax = max of the selected scores).  Native: a radix
        select, ties at the B-th value to the lower row index, NaN above every number and etpmax NaN then; the torch
        path is np.argpartition's choice."""
        return self._timed("select", lambda: self._select(etp, X, B))

    def _select(self, etp, X, B):
        n = X.shape[0]
        if B > n:
            raise ValueError("B exceeds the pool (the caller clamps B to the pool's remainder)")
        if B == 0:
            return dict(idx=np.zeros(0, dtype=np.int64), scores=np.zeros(0), X_sel=X[:0], X_rest=X, etpmax=0.0)
        if self.native:
            import ctypes
            X = self._dev_rows(X, torch.float64, self.nin, "the pool")
            etp = self._dev_rows(etp, torch.float32, None, "etp")
            if etp.shape[0] != n:
                raise ValueError("etp and the pool differ in their row counts")
            idx = torch.empty((B,), dtype=torch.int64, device=self.device)
            X_sel = torch.empty((B, self.nin), dtype=torch.float64, device=self.device)
            X_rest = torch.empty((n - B, self.nin), dtype=torch.float64, device=self.device)
            mx = ctypes.c_float()
            ptr = lambda t: t.data_ptr() if t.numel() else None
            self._pl.check(self._lib.vboc_pool_select(self._h, ptr(etp), ptr(X), n, B, self.nin, ptr(idx), ptr(X_sel),
                                                      ptr(X_rest), ctypes.byref(mx), self._stream()))
            return dict(idx=idx.cpu().numpy(), scores=etp[idx].cpu().numpy(), X_sel=X_sel, X_rest=X_rest,
                        etpmax=float(mx.value))
        maxindex = np.argpartition(etp, -B)[-B:].tolist()
        maxindex.sort(reverse=True)
        etpmax = max(etp[maxindex])
        idx = np.asarray(maxindex, dtype=np.int64)
        return dict(idx=idx, scores=etp[idx], X_sel=X[idx], X_rest=np.delete(X, idx, 0), etpmax=float(etpmax))

    # -- the guess network's trajectories (compute_problem_nnguess) -----------------------------------
    @torch.no_grad()
    def guess(self, X0, N, mean, std):
        """x_guess [B, N + 1, 2nq] float64 for the states X0 [B, 2nq]: stage 0 = x0, stages 1..N the network's output
        * std + mean.  Native: a device tensor; torch path: al.nn_guess per state, a NumPy array."""
        return self._timed("guess", lambda: self._guess(X0, N, mean, std))

    def _guess(self, X0, N, mean, std):
        Bq = X0.shape[0]
        if self.native:
            outputs = self.guess_model.linear_relu_stack[4].out_features
            if not self._pl.supported(self.nin, self.hidden, outputs) or outputs != self.nin * N:
                raise ValueError(f"libvboc_pool.so does not implement guess outputs {outputs} for N {N}")
            X0 = self.to_pool(X0)
            xg = torch.empty((Bq, N + 1, self.nin), dtype=torch.float64, device=self.device)
            if Bq:
                self._pl.check(self._lib.vboc_pool_set_guess(self._h, outputs, *self._ptrs(self.guess_model),
                                                             self._stream()))
                self._pl.check(self._lib.vboc_pool_guess(self._h, X0.data_ptr(), Bq, N, float(mean), float(std),
                                                         xg.data_ptr(), self._stream()))
            return xg
        from .al import nn_guess
        X0 = np.asarray(X0, dtype=np.float64)
        n = self.nq
        mean_t = torch.as_tensor(mean, dtype=torch.float32).to(self.device)
        std_t = torch.as_tensor(std, dtype=torch.float32).to(self.device)
        return np.stack([nn_guess(N, s[:n], s[n:], self.guess_model, mean_t, std_t) for s in X0]) if Bq else \
            np.zeros((0, N + 1, 2 * n))


class GuessTrainer:
    """The guess network of the AL loop on PyTorch: NeuralNetCLS(2nq, hidden, 2nq N), MSELoss, Adam(lr), one
    optimizer for the whole run; fit() is `while val > loss_stop and it <= it_max` with val from 1
    (AL/triplependulum_al.py:172-200, :353-387).  Rows of a fit: a labelled-viable state's trajectory, (N + 1) 2nq
    values: the state, then the targets; both are normalised with (. - mean) / std in float32.  seed=None leaves
    torch's generator where it is (the reference builds this model right after the classifier); rng is the
    random.Random both fits of the loop share."""

    def __init__(self, nq, N, device="cpu", hidden=100, lr=1e-3, beta=0.95, stop_val=0.1, seed=None, rng=None):
        import random
        self.nq, self.nin, self.N = nq, 2 * nq, N
        self.device = torch.device(device)
        if seed is not None:
            torch.manual_seed(seed)
        self.hidden = hidden
        self.model = NeuralNetCLS(self.nin, hidden, self.nin * N).to(self.device)
        self.lr, self.beta, self.stop_val = lr, beta, stop_val
        self.opt = torch.optim.Adam(self.model.parameters(), lr=lr)
        self.crit = nn.MSELoss()
        self.rng = rng if rng is not None else random.Random(seed)
        self.total_steps = 0
        self.last = None

    def fit(self, T, mean, std, it_max, qt, max_steps=None):
        """T [m, (N + 1) 2nq] float64 trajectories; qt the minibatch size asked for (clamped to m inside the loop, as
        :180-181).  max_steps caps the steps below the reference's rule (measurements).  Returns dict(iterations,
        val, qt)."""
        T = np.asarray(T, dtype=np.float64).reshape(-1, (self.N + 1) * self.nin)
        mean_t = torch.as_tensor(mean, dtype=torch.float32).to(self.device)
        std_t = torch.as_tensor(std, dtype=torch.float32).to(self.device)
        T32 = torch.from_numpy(T.astype(np.float32)).to(self.device)
        it, val = 0, 1
        while val > self.stop_val and it <= it_max and (max_steps is None or it < max_steps):
            if T.shape[0] < qt:
                qt = T.shape[0]
            ind = torch.as_tensor(self.rng.sample(range(T.shape[0]), qt), dtype=torch.long, device=self.device)
            X_iter_tensor = T32[ind, :self.nin]
            y_iter_tensor = T32[ind, self.nin:]
            X_iter_tensor = (X_iter_tensor - mean_t) / std_t
            y_iter_tensor = (y_iter_tensor - mean_t) / std_t
            outputs = self.model(X_iter_tensor)
            loss = self.crit(outputs, y_iter_tensor)
            loss.backward()
            self.opt.step()
            self.opt.zero_grad()
            val = self.beta * val + (1 - self.beta) * loss.item()
            it += 1
        self.total_steps += it
        self.last = dict(iterations=it, val=val, qt=qt)
        return dict(self.last)
