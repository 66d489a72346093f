"""An objective on which both optimisers can be held to float64, iterate by iterate.  TEST INFRASTRUCTURE (numpy only).

With an empty weight table only the image terms of the objective remain (worker.py:283-297), and with tv_power = p_power = 2 they are
an exact quadratic in x: k == 1 in ``oracle.image_norms.tv_term``, the gradient is linear and the Hessian in x, (tv L + p I) / 255^2,
is symmetric positive-definite (L: the periodic Laplacian-like stencil of tv_term).  The optimisers are handed the gradient without the
1/255 chain factor, so the linear map they see is (tv L + p I) / 255.  A fixed-step L-BFGS contracts on it, so rounding is
not amplified, and a float64 run of the same algorithm is a reference every iterate can be compared with -- through evictions, gate
rejections and a cleared history.  ``LBFGS64`` / ``Adam64`` restate ``oracle.descent.LBFGSOracle`` / ``AdamOracle`` in float64
(np.vdot: scipy's sdot would round to fp32); tests/test_quadratic_oracle_cpu.py holds the fp32 oracles to them and shows that the bars
the GPU tests use separate every mutant in ``MUTANTS`` from rounding.
"""
import functools

import numpy as np

from oracle import descent, image_norms

F32, F64 = np.float32, np.float64

JOB = dict(seed=5, tv=5, p=1, tv_power=2, p_power=2)
SCHEDULE = {
    # fixed step 0.5; a step of 1e-9 moves an fp32 x at most at the few pixels that are nearly zero (tiny_step_effect), so y = 0 or
    # nearly so and the pair is rejected (in float64 s.y ~ 1e-17)
    'lbfgs': dict(step=0.5, steps=36, tiny_step=1e-9, tiny_at=(13, 14, 25)),
    # a replacement input (seed 6) together with objective_changed before step 12, a quarter of the step size from step 20 on
    'adam': dict(step=10, steps=30, new_input_at=12, new_input_seed=6, late_step=2.5, late_from=20),
    # the second grid sweep of the device kernels (3 h w / 4 > 1024 x 256): past the first eviction, one rejection
    'lbfgs_big': dict(step=0.5, steps=14, tiny_step=1e-9, tiny_at=(12,)),
}
SIZES = ((15, 17), (64, 96))          # 3 h w % 4 = 1 (scalar tail of the device kernels) and 0 (float4 body)
BIG_SIZE = (592, 600)                 # 3 h w / 4 = 266 400 > 262 144 float4 lanes of one sweep
GATE = 1e-10                          # optimizers.py:82

X_ATOL = 0.02         # max |x_dev - x_64| in preprocessed pixel units (x starts at +-135): > 10 x the fp32 oracle's own 1.6e-3, 10 x below
                      # the smallest mutant (0.2); both measured on the CPU by tests/test_quadratic_oracle_cpu.py.  Measured on an MI355X
                      # by tests/test_gpu_quadratic_descent.py: 1.15e-3 (15x17) ... 2.53e-3 (592x600), all three forms
# Relative loss bar: ten times the worst deviation of the fp32 oracle from float64 over the L-BFGS runs at SIZES and BIG_SIZE, rounded
# up to one digit.  Measured 3.4e-4 (15x17, step 34, where the loss is 7e-5 and dominated by the 1e-8 floor inside tv_term); 64x96:
# 4.3e-5; 592x600: 1.7e-6.
LOSS_RTOL = 4e-3
# s.y of every pair the schedule means to keep / to reject lies beyond these, so no gate decision is near GATE.  At BIG_SIZE the
# rejected pair has s.y = 2.3e-13 in float64 (1.1e-15 in fp32): s.y scales with the 1.1e6 pixels, and no step of a 14-step run brings
# it below 1e-14 -- the rejection stays at step 12 and the bar for that size is 1e-12, still a factor 100 from the gate.
SY_KEPT_MIN, SY_REJECTED_MAX, SY_REJECTED_MAX_BIG = 1e-6, 1e-14, 1e-12
ADAM_X_ATOL = 0.05    # CPU, fp32 Adam oracle against float64: 2.06e-4 (64x96), 2.6e-5 (15x17).  MI355X, the engine against float64: 2.06e-4
                      # and 2.56e-5.  Mutants of the clearing rules sit at 58 and above, so the bar is far from both
ADAM_M_RTOL, ADAM_V_RTOL = 1e-3, 1e-5     # max-relative, after steps ADAM_STATE_STEPS (CPU fp32 oracle: 4e-7 and 6e-7; MI355X: 4.0e-7 and 6.4e-7)
ADAM_STATE_STEPS = (11, 12, 19, 29)


def x0(h, w, seed=JOB['seed']):
    return (np.random.RandomState(seed).rand(1, 3, h, w) * 255 - 120).astype(F32)


def objective(x, tv=JOB['tv'], p=JOB['p'], dtype=F64):
    """(loss, grad) of the image-terms-only objective, combined as TransferOracle.opfunc combines them (no 1/255 chain factor)."""
    u = np.asarray(x, dtype) / dtype(255)
    tv_value, tv_grad = image_norms.tv_term(u, 2)
    p_value, p_grad = image_norms.p_term(u, 2)
    loss = dtype(tv) * tv_value + dtype(p) * p_value
    grad = dtype(tv) * tv_grad + dtype(p) * p_grad
    assert grad.dtype == dtype and np.asarray(loss).dtype == dtype
    return loss, grad


def opfunc(dtype):
    return lambda x: objective(x, dtype=dtype)


class LBFGS64:
    """oracle.descent.LBFGSOracle in float64.  ``log`` has one (s.y, kept, pair count) per step.  The keyword arguments are the
    mutations of MUTANTS; the defaults are the algorithm."""

    def __init__(self, x, opfunc, step_size=1, n_corr=10, evict=0, gate=GATE, h0_pair=-1):
        self.x, self.opfunc, self.step_size = np.array(x, F64), opfunc, step_size
        self.n_corr, self.evict, self.gate, self.h0_pair = n_corr, evict, gate, h0_pair
        self.loss = self.grad = None
        self.pairs = []          # (s, y, s.y), oldest first
        self.log = []

    def step(self):
        if self.loss is None:
            self.loss, self.grad = self.opfunc(self.x)
        s = -self.step_size * self.inv_hessian_times(self.grad)
        self.x += s
        loss, grad = self.opfunc(self.x)
        y = grad - self.grad
        sy = float(np.vdot(s, y))
        kept = sy > self.gate
        if kept:
            self.pairs.append((s, y, sy))
        if len(self.pairs) > self.n_corr:
            del self.pairs[self.evict]
        self.loss, self.grad = loss, grad
        self.log.append((sy, kept, len(self.pairs)))
        return self.x, loss

    def inv_hessian_times(self, p):
        p = p.copy()
        alphas = []
        for s, y, sy in reversed(self.pairs):
            alphas.append(np.vdot(s, p) / sy)
            p -= alphas[-1] * y
        if self.pairs:
            _, y, sy = self.pairs[self.h0_pair]
            p *= sy / np.vdot(y, y)
        else:
            p /= np.sqrt(np.vdot(p, p) / p.size)
        for (s, y, sy), alpha in zip(self.pairs, reversed(alphas)):
            beta = np.vdot(y, p) / sy
            p += (alpha - beta) * s
        return p

    def objective_changed(self):
        self.pairs = []
        self.loss = self.grad = None


MUTANTS = {
    'evict newest instead of oldest': dict(evict=-2),          # (the pair in front of the one just stored)
    'evict second-oldest': dict(evict=1),
    'n_corr = 9': dict(n_corr=9),
    'n_corr = 11': dict(n_corr=11),
    'gate s.y > 0': dict(gate=0.0),
    'H0 scale from the oldest pair': dict(h0_pair=0),
}


class Adam64:
    """oracle.descent.AdamOracle in float64: ``m`` / ``v`` are the uncorrected running means, ``items1`` / ``items2`` their counts."""

    def __init__(self, x, opfunc, step_size=1, b1=0.9, b2=0.999):
        self.x, self.opfunc, self.step_size, self.b1, self.b2 = np.array(x, F64), opfunc, step_size, b1, b2
        self.m = np.zeros_like(self.x)
        self.v = np.zeros_like(self.x)
        self.items1 = self.items2 = 0

    def step(self):
        loss, grad = self.opfunc(self.x)
        self.m = self.b1 * self.m + (1 - self.b1) * grad
        self.v = self.b2 * self.v + (1 - self.b2) * grad**2
        self.items1 += 1
        self.items2 += 1
        m_hat = self.m / (1 - self.b1**self.items1)
        v_hat = self.v / (1 - self.b2**self.items2)
        self.x -= self.step_size * m_hat / (np.sqrt(v_hat) + 1e-8)
        return self.x, loss

    def objective_changed(self):
        self.m = np.zeros_like(self.x)
        self.items1 = 0


def lbfgs_step_size(k, sched):
    return sched['tiny_step'] if k in sched['tiny_at'] else sched['step']


def run_lbfgs(opt, sched, events=None):
    """The scheduled run on any optimiser with LBFGSOracle's interface: [(x copy, loss)] per step.  events = {step: callable(opt)} run
    before that step (a replacement input, objective_changed)."""
    out = []
    for k in range(sched['steps']):
        if events and k in events:
            events[k](opt)
        opt.step_size = lbfgs_step_size(k, sched)
        x, loss = opt.step()
        out.append((x.copy(), float(loss)))
    return out


class Logged32(descent.LBFGSOracle):
    """The fp32 oracle with LBFGS64's ``log``: s and y are recomputed beside the unchanged step (both are deterministic)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.log = []

    def step(self):
        if self.loss is None:
            self.loss, self.grad = self.opfunc(self.x)
        s = -self.step_size * self.inv_hessian_times(self.grad)
        g_old, before = self.grad, len(self.pairs)
        newest = self.pairs[-1] if self.pairs else None
        out = super().step()
        sy = float(descent.sdot(s, self.grad - g_old))
        kept = bool(self.pairs) and self.pairs[-1] is not newest
        assert kept == (sy > GATE) and len(self.pairs) == min(before + kept, self.n_corr)
        self.log.append((sy, kept, len(self.pairs)))
        return out


def rejected_steps(log):
    return tuple(k for k, (_, kept, _) in enumerate(log) if not kept)


def assert_events(log, sched, rejected_max=SY_REJECTED_MAX, tag=''):
    """The events the schedule is meant to produce, in a ``log`` of an uninterrupted run: ten pairs from step 9 on, rejections exactly
    at the tiny steps, no s.y anywhere near the gate."""
    counts = [n for _, _, n in log]
    kept = [sy for sy, k, _ in log if k]
    dropped = [sy for sy, k, _ in log if not k]
    print('[%s] smallest kept s.y %.3g, largest rejected s.y %.3g' % (tag, min(kept), max(dropped)))
    assert counts[:9] == list(range(1, 10)) and all(n == 10 for n in counts[9:]), counts
    assert rejected_steps(log) == tuple(sched['tiny_at']), rejected_steps(log)
    assert min(kept) > SY_KEPT_MIN and max(dropped) < rejected_max, (min(kept), max(dropped))


def tiny_step_effect(ref, k):
    """What a rejected step may do to an fp32 iterate, from the float64 run `ref` = [(x, loss)]: (max |s|, may_move).  fl(x + s) differs
    from x only where |s| >= ulp(x) / 2 and then by at most 2 |s|; may_move is False where every |s| is below a quarter ulp, so that
    no correctly rounded implementation moves any pixel and the iterate must stay bit-identical."""
    s = np.abs(ref[k][0] - ref[k - 1][0])
    ulp = np.spacing(np.abs(ref[k - 1][0]).astype(F32)).astype(F64)
    return float(s.max()), bool((s >= ulp / 4).any())


def lbfgs_reference(h, w, sched=None, events=None, **mutation):
    """[(x, loss)] and the log of LBFGS64 (or a mutant of it) on the job at h x w."""
    sched = sched or SCHEDULE['lbfgs']
    opt = LBFGS64(x0(h, w), opfunc(F64), sched['step'], **mutation)
    return run_lbfgs(opt, sched, events), opt.log


def lbfgs_fp32(h, w, sched=None):
    sched = sched or SCHEDULE['lbfgs']
    opt = Logged32(x0(h, w), opfunc(F32), sched['step'])
    return run_lbfgs(opt, sched), opt.log


def run_adam(opt, h, w, sched=None, state_of=None):
    """The Adam half of the job: [(x copy, loss)] per step and {step: state_of(opt)} after the steps of ADAM_STATE_STEPS."""
    sched = sched or SCHEDULE['adam']
    out, states = [], {}
    for k in range(sched['steps']):
        if k == sched['new_input_at']:
            opt.x[:] = x0(h, w, sched['new_input_seed'])
            opt.objective_changed()
        opt.step_size = sched['late_step'] if k >= sched['late_from'] else sched['step']
        x, loss = opt.step()
        out.append((x.copy(), float(loss)))
        if state_of and k in ADAM_STATE_STEPS:
            states[k] = state_of(opt)
    return out, states


def adam_reference(h, w):
    opt = Adam64(x0(h, w), opfunc(F64), SCHEDULE['adam']['step'])
    return run_adam(opt, h, w, state_of=lambda o: (o.m.copy(), o.v.copy(), o.items1, o.items2))


def adam_fp32(h, w):
    opt = descent.AdamOracle(x0(h, w), opfunc(F32), SCHEDULE['adam']['step'])
    return run_adam(opt, h, w, state_of=lambda o: (np.array(o.g1.mean), np.array(o.g2.mean), o.g1.items, o.g2.items))


def max_abs(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max())


def max_rel(a, b):
    """max |a - b| relative to max |b|."""
    return max_abs(a, b) / float(np.abs(b).max())


CLEARED = dict(at=21, seed=6, more=16)     # the history dropped in mid-run: a new input and objective_changed after step 20, 16 more steps


@functools.lru_cache(maxsize=None)
def reference(kind, h, w):
    """The float64 runs the tests share, computed once per session and never modified: 'lbfgs' and 'lbfgs_big' -> ([(x, loss)], log),
    'lbfgs_cleared' -> the same for the run of CLEARED, 'adam' -> ([(x, loss)], {step: (m, v, items1, items2)})."""
    if kind == 'adam':
        out = adam_reference(h, w)
    elif kind == 'lbfgs_cleared':
        def replace(opt):
            opt.x[:] = x0(h, w, CLEARED['seed'])
            opt.objective_changed()
        sched = dict(SCHEDULE['lbfgs'], steps=CLEARED['at'] + CLEARED['more'])
        out = lbfgs_reference(h, w, sched, {CLEARED['at']: replace})
    else:
        out = lbfgs_reference(h, w, SCHEDULE[kind])
    for x, _ in out[0]:
        x.flags.writeable = False
    return out
