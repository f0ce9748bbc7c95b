"""Adam with the loss scale of fp16 training kept on the device (csrc/optim.hip).

The reference trains with torch.optim.Adam(lr=1e-4, amsgrad=True, weight_decay=1e-4) (scripts/simple_train.py:121).  NativeAdam
is that update plus what torch splits between the optimizer and a GradScaler — the non-finite check of the gradients, the
division by the loss scale S, the skipped step and the growth / backoff of S — as launches that only enqueue: torch's
GradScaler protocol (unscale_ / step / update) synchronises with the host or reaches into private attributes of the fused
optimizer, and the Trainer's whole step is one hipGraph.

    opt = NativeAdam(params, lr=1e-4, weight_decay=1e-4, loss_scale='dynamic')
    loss.backward(gradient=opt.loss_scale)          # the device scalar S seeds the backward pass: no extra multiply
    opt.step()                                      # check, (un-scaled) Adam or nothing, S update

max_grad_norm=M adds what torch.nn.utils.clip_grad_norm_ does, inside the same step: the check's pass also takes the global sum of
squares, and Adam reads grad / S * min(M / (norm + 1e-6), 1); opt.grad_norm is the pre-clip norm as a device scalar.

state_dict() has torch.optim.Adam's layout (state keys step / exp_avg / exp_avg_sq / max_exp_avg_sq, the same param_groups
entries), so a checkpoint moves between the two in both directions; the scale's own state travels separately
(scaler_state_dict), as a GradScaler's does.
"""
import math
import numbers

import torch

from . import ops
from ._lib import UpflowHipError

DYNAMIC_INIT_SCALE = 2.0 ** 16                       # torch.amp.GradScaler's defaults: init_scale, growth_interval = 2000,
                                                     # growth_factor = 2, backoff_factor = 0.5


def parse_loss_scale(loss_scale):
    """-> (initial scale, dynamic?) of a `loss_scale` argument: 'dynamic', or a fixed positive power of two (the division by it is
    then exact); anything else is a ValueError."""
    if isinstance(loss_scale, str):
        if loss_scale != 'dynamic':
            raise ValueError("loss_scale must be None, 'dynamic' or a positive power of two, got %r" % (loss_scale,))
        return DYNAMIC_INIT_SCALE, True
    s = float(loss_scale)
    if not (math.isfinite(s) and s > 0 and math.frexp(s)[0] == 0.5 and 2.0 ** -126 <= s <= 2.0 ** 127):
        raise ValueError("loss_scale must be None, 'dynamic' or a positive power of two (fp32 range), got %r" % (loss_scale,))
    return s, False


def parse_max_grad_norm(max_grad_norm):
    """-> None, or the bound as a python float: a positive number or math.inf (measure the norm, clip nothing); anything else —
    <= 0, NaN, a non-number — is a ValueError."""
    if max_grad_norm is None:
        return None
    if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, numbers.Real) or not float(max_grad_norm) > 0.0:
        raise ValueError('max_grad_norm must be None, a positive number or math.inf, got %r' % (max_grad_norm,))
    return float(max_grad_norm)


class NativeAdam(torch.optim.Optimizer):
    """torch.optim.Adam(amsgrad=True, weight_decay=L2) whose step is three kernel families on the current stream — no host
    synchronisation, no .item() — with a loss scale:
        loss_scale   'dynamic' (starts at 2^16, halves on a non-finite step, never below 1, doubles after growth_interval clean
                     steps), or a fixed power of two (default 1.0: plain Adam that skips non-finite steps)
        max_grad_norm  None (default): the step above, launch for launch.  A positive float: the global L2 norm of the UN-scaled
                     gradients of ALL groups is bounded as torch.nn.utils.clip_grad_norm_ bounds it — coef = min(max_grad_norm /
                     (norm + 1e-6), 1) — inside the step: the non-finite pass also takes the sum of squares (double, fixed order, no
                     atomics: reproducible), one workgroup turns it into `grad_norm` and `clip_coef`, and Adam multiplies the
                     coefficient in where it reads the gradient.  p.grad itself is NOT modified, unlike torch: the coefficient is
                     folded into the read.  math.inf: the norm is measured, nothing is clipped (clip_coef == 1 exactly).  On a
                     non-finite step grad_norm is non-finite (if and only if) and clip_coef is unspecified.  No state: state_dict()
                     is unchanged.
    Device tensors: loss_scale (fp32, the seed for loss.backward), skipped_steps, growth_tracker (int32); with max_grad_norm
    grad_norm (fp32: the pre-clip norm of the un-scaled gradients of the last step) and clip_coef (fp32).
    lr may be a python float or a device tensor (graph capture: a tensor, updated in place by the schedulers)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=True, *, loss_scale=1.0,
                 growth_interval=2000, growth_factor=2.0, backoff_factor=0.5, max_grad_norm=None):
        max_grad_norm = parse_max_grad_norm(max_grad_norm)
        if not amsgrad:
            raise ValueError('NativeAdam implements the amsgrad variant only (scripts/simple_train.py:121)')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0 and weight_decay >= 0.0):
            raise ValueError('betas in [0, 1), eps >= 0, weight_decay >= 0')
        if not torch.is_tensor(lr) and lr < 0.0:
            raise ValueError('invalid learning rate %r' % (lr,))
        init, dynamic = parse_loss_scale(loss_scale)
        if dynamic and not (int(growth_interval) >= 1 and growth_factor >= 1.0 and 0.0 < backoff_factor <= 1.0):
            raise ValueError('growth_interval >= 1, growth_factor >= 1, 0 < backoff_factor <= 1')
        # torch.optim.Adam's own param_groups keys (whatever this torch version has), so that state dicts interchange;
        # fused / capturable say what is true of this step: one multi-tensor pass that reads lr and step on the device and does not
        # advance the parameters' autograd version counters (ops.register_version_hook keys on `fused`)
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=True, maximize=False, foreach=None,
                        capturable=True, differentiable=False, fused=True)
        super().__init__(params, defaults)
        first = self.param_groups[0]['params'][0]
        if not first.is_cuda:
            raise UpflowHipError('NativeAdam runs on the GPU only (got a %s parameter); there is no CPU path' % first.device)
        dev = first.device
        self.dynamic = dynamic
        self.growth_interval = int(growth_interval) if dynamic else 0          # (0: the kernel leaves the scale alone)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.loss_scale = torch.tensor(init, dtype=torch.float32, device=dev)
        self.growth_tracker = torch.zeros((), dtype=torch.int32, device=dev)
        self.skipped_steps = torch.zeros((), dtype=torch.int32, device=dev)
        self._flag = torch.zeros((), dtype=torch.int32, device=dev)
        self._steps = torch.zeros(len(self.param_groups), dtype=torch.float32, device=dev)   # one counter per group
        self._lr_dev = [None] * len(self.param_groups)                          # (device copies of python-float learning rates)
        self._tables = {}
        self.max_grad_norm = max_grad_norm
        if max_grad_norm is not None:
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            self.clip_coef = torch.ones((), dtype=torch.float32, device=dev)
            self._partials = None                                # (fp64, one per workgroup of all groups: made with the tables)

    def add_param_group(self, group):
        super().add_param_group(group)
        if hasattr(self, '_steps') and len(self.param_groups) > self._steps.numel():
            self._steps = torch.cat([self._steps, self._steps.new_zeros(len(self.param_groups) - self._steps.numel())])
            self._lr_dev.append(None)
            self._relink_steps()
            self._tables = {}

    def _relink_steps(self):
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                if p in self.state:
                    self.state[p]['step'] = self._steps[gi]

    def load_state_dict(self, state_dict):
        """Also from a torch.optim.Adam(amsgrad=True): its per-parameter step counts (host or device) become this optimizer's
        per-group device counter (the count of the group's first parameter)."""
        super().load_state_dict(state_dict)
        for gi, group in enumerate(self.param_groups):
            if not group.get('amsgrad', False) or group.get('maximize', False):
                raise ValueError('NativeAdam: the loaded param_groups must have amsgrad=True, maximize=False')
            group.update(capturable=True, fused=True, foreach=None, differentiable=False)
            for p in group['params']:
                st = self.state.get(p)
                if st:
                    if 'max_exp_avg_sq' not in st:
                        raise ValueError('NativeAdam: the loaded state has no max_exp_avg_sq (not an amsgrad state)')
                    self._steps[gi].copy_(torch.as_tensor(st['step'], dtype=torch.float32).reshape(()), non_blocking=True)
                    break
        self._relink_steps()
        self._tables = {}

    def state_dict(self):
        """torch.optim.Adam's layout; every parameter gets a step tensor of its own (the group's counter, copied), as torch's
        states have: the views into the shared counter would stay aliased through a save / load."""
        sd = super().state_dict()
        sd['state'] = {k: dict(v, step=v['step'].clone()) for k, v in sd['state'].items()}
        return sd

    def scaler_state_dict(self):
        """The loss scale's state as python numbers (synchronises: checkpoint time only)."""
        return {'loss_scale': float(self.loss_scale), 'growth_tracker': int(self.growth_tracker), 'skipped_steps': int(self.skipped_steps)}

    def load_scaler_state_dict(self, d):
        self.loss_scale.fill_(parse_loss_scale(d['loss_scale'])[0])
        self.growth_tracker.fill_(int(d['growth_tracker']))
        self.skipped_steps.fill_(int(d['skipped_steps']))

    def _group_tables(self, gi, group):
        """The launch tables of group gi for the parameters that have a gradient now (state made on first sight, as torch does)."""
        params = [p for p in group['params'] if p.grad is not None]
        if not params:
            return None
        key = tuple(id(p) for p in params)
        cached = self._tables.get(gi)
        if cached is None or cached[0] != key:
            for p in params:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise UpflowHipError('NativeAdam: parameters must be contiguous fp32 tensors')
                st = self.state[p]
                if not st:
                    st['step'] = self._steps[gi]
                    for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
                        st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            t = ops.MtTables([p.numel() for p in params])
            t.set('param', [p.data for p in params])
            for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
                t.set(k, [self.state[p][k] for p in params])
            cached = (key, t)
            self._tables[gi] = cached
        cached[1].set('grad', [p.grad for p in params])       # (new addresses every eager step; fixed inside a captured one)
        return cached[1]

    def _lr_tensor(self, gi, group):
        lr = group['lr']
        if torch.is_tensor(lr):
            if lr.is_cuda and lr.dtype == torch.float32:
                return lr
            lr = float(lr)
        held = self._lr_dev[gi]
        if held is None or held[0] != lr:                      # a python float: its device copy is refreshed when it changes
            buf = held[1] if held is not None else torch.empty((), dtype=torch.float32, device=self._steps.device)
            buf.fill_(lr)
            held = self._lr_dev[gi] = (lr, buf)
        return held[1]

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise UpflowHipError('NativeAdam.step takes no closure (the step only enqueues kernels)')
        work = [(gi, g, self._group_tables(gi, g)) for gi, g in enumerate(self.param_groups)]
        work = [w for w in work if w[2] is not None]
        if not work:
            return None
        if self.max_grad_norm is not None:
            return self._clipped_step(work)
        for _, _, t in work:                                   # 1. ANY non-finite gradient of ANY group skips the whole step
            ops.grads_nonfinite_check(t, self._flag)
        for gi, g, t in work:                                  # 2. the update, or nothing
            ops.adam_amsgrad_step(t, self._lr_tensor(gi, g), self._steps[gi], self.loss_scale, self._flag, g['betas'][0],
                                  g['betas'][1], g['eps'], g['weight_decay'])
        # 3. step counters, scale, tracker, skipped count; clears the flag
        ops.loss_scale_update(self.loss_scale, self.growth_tracker, self.skipped_steps, self._flag, self._steps,
                              self.growth_factor, self.backoff_factor, self.growth_interval)
        return None

    def _clipped_step(self, work):
        n = sum(t.n_blocks for _, _, t in work)
        if self._partials is None or self._partials.numel() != n:
            # allocated when the tables are (re)built — the eager warm-up steps — so that a captured step reads a fixed address
            self._partials = torch.zeros(n, dtype=torch.float64, device=self._steps.device)
        off = 0
        for _, _, t in work:                                   # 1. the non-finite check and the sum of squares, one pass
            off += ops.grads_sumsq_check(t, self._partials[off:off + t.n_blocks], self._flag)
        # 2. the norm of the un-scaled gradients and the coefficient (one workgroup)
        ops.grad_norm_clip_coef(self._partials, self.loss_scale, self.max_grad_norm, self.grad_norm, self.clip_coef)
        for gi, g, t in work:                                  # 3. the update on grad / S * coef, or nothing
            ops.adam_amsgrad_step(t, self._lr_tensor(gi, g), self._steps[gi], self.loss_scale, self._flag, g['betas'][0],
                                  g['betas'][1], g['eps'], g['weight_decay'], clip_coef=self.clip_coef)
        # 4. step counters, scale, tracker, skipped count; clears the flag
        ops.loss_scale_update(self.loss_scale, self.growth_tracker, self.skipped_steps, self._flag, self._steps,
                              self.growth_factor, self.backoff_factor, self.growth_interval)
        return None
