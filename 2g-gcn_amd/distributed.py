"""Batch data-parallel training of the 2G-GCN path: one process per GPU, gradients summed with ONE collective family
(all-reduce over RCCL/xGMI through torch.distributed, backend "nccl" == RCCL on ROCm; "gloo" in the CPU tests).

The reference has no distributed code at all; clips are independent, so the only exchange step is the
gradient all-reduce (45.5 M fp32 for the MPHOI/C3 model = 182 MB). Design for xGMI (point-to-point links, ring
collectives are per-link bound): all parameters live in ONE flat fp32 buffer and all gradients in another, so the step
issues a handful of large all-reduces (chunks of `bucket_mb`) instead of 100+ small ones, and the 1/world_size
averaging is folded into the fused Adam kernel (no extra pass over the gradients).

BatchNorm statistics of the geometry branch stay local to each rank (standard DDP semantics); Gumbel noise is drawn
per rank. Dead parameters (constructed by the reference but never used) keep a zero gradient.
The three cross-sample couplings of SURVEY 8e have an exact-equivalence switch each: sync_bn (a), count_weighted_loss
(b), global_noise_seed or device_noise_seed (c).
"""
import contextlib
import os
import weakref

import torch
import torch.distributed as dist

from .kernels import get_kernels


def _remove_installed(model, installed):
    """Removes from the model's side table exactly the objects in `installed` (key -> object): an entry a LATER wrapper of
    the same model put there under the same key is somebody else's and stays."""
    from . import ops
    for key, obj in installed.items():
        if ops.get_model_extra(model, key) is obj:
            ops.set_model_extra(model, key, None)


def _drop_extras(model_ref, wrapper_ref, installed):
    """weakref.finalize callback of a collected DataParallel: removes what THAT wrapper left beside a model that is still
    alive. A re-wrap (`dp = DataParallel(model, ...)` rebinding `dp`) constructs the new wrapper before the old one is
    collected; the old one's finalizer must not take the new one's sync-BN reducer / noise shard with it."""
    model = model_ref()
    if model is None:
        return
    from . import ops
    hook = ops.get_model_extra(model, 'stage_hook')
    if isinstance(hook, weakref.WeakMethod) and hook() is None:
        ops.set_grad_stage_hook(model, None)
    _remove_installed(model, installed)


class FlatParameters:
    """Re-homes every parameter of `module` as a view into one flat buffer; same for the gradients."""

    def __init__(self, module: torch.nn.Module, stage_of=None, extra_modules=()):
        """stage_of (optional): name -> int; parameters are laid out by ascending stage (stable), and
        `stage_ranges[stage] = (begin, end)` gives each stage's slice of the flat buffers.
        extra_modules: further modules (the multi-task loss learner) whose parameters follow the model's, in a stage of
        their own after the model's last one. `module_ranges[0]` is the model's (begin, end) slice, `module_ranges[1 + j]`
        that of extra_modules[j]."""
        named = list(module.named_parameters())
        # (name, parameter) in named_parameters() order, the model first, then each extra module: the layout below sorts by
        # stage, an optimizer checkpoint (FusedAdam.state_dict) is in this order
        self.named_groups = [list(named)] + [list(m.named_parameters()) for m in extra_modules]
        if stage_of is not None:
            named.sort(key=lambda kv: stage_of(kv[0]))
        groups = [named] + [list(m.named_parameters()) for m in extra_modules]
        params = [p for g in groups for _, p in g]
        if len({id(p) for p in params}) != len(params):
            raise ValueError('a parameter belongs to the model and to an extra module (or to two extra modules)')
        dev = params[0].device
        sizes = [(p.numel() + 3) // 4 * 4 for p in params]  # keep every view 16-byte aligned for the kernels
        total = sum(sizes)
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p, n in zip(params, sizes):
                view = self.flat[off:off + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[off:off + p.numel()].view_as(p)
                off += n
        self.params = params
        from . import ops
        ops.enable_grad_sinks(params)   # the backward kernels add straight into these flat gradient views
        self.numel = total
        self.module_ranges = []
        off = k = 0
        for g in groups:
            b = off
            for _ in g:
                off += sizes[k]
                k += 1
            self.module_ranges.append((b, off))
        self.stage_ranges = {}
        if stage_of is not None:
            off = 0
            for (name, _), n in zip(named, sizes):
                st = stage_of(name)
                b, _e = self.stage_ranges.get(st, (off, off))
                self.stage_ranges[st] = (b, off + n)
                off += n
            if len(groups) > 1:   # the extra modules' gradients are final as soon as the backward pass begins
                self.stage_ranges[max(self.stage_ranges, default=-1) + 1] = (self.module_ranges[1][0], total)

    def zero_grad(self):
        K = get_kernels()
        if hasattr(K, 'fill_zero') and self.grad.is_cuda:
            K.fill_zero(self.grad)   # the library's clear (no ATen fill on the step's path)
        else:
            self.grad.zero_()
        for p in self.params:  # autograd accumulates in place into these views
            if p.grad is None or p.grad.data_ptr() == 0:
                raise RuntimeError('parameter lost its flat gradient view')


class FusedAdam:
    """torch.optim.Adam semantics (reference train.py:39) as one fused kernel over the flat buffers.

    max_grad_norm > 0: the reference's `clip_gradient_at` (train_utils.py:149-153), torch.nn.utils.clip_grad_norm_ over the
    MODEL's parameters between backward() and step(), folded into the step: one norm over the model's slice of the (already
    all-reduced) gradient buffer, measured on the averaged gradient g * grad_scale, then Adam reading the clip coefficient
    from the device. The slices of extra modules (FlatParameters(extra_modules=...): the loss learner) are stepped without
    it. step() then returns the pre-clip norm as a 0-d device tensor (what clip_grad_norm_ returns); nothing is read on
    the host.

    The device path. Any of decoupled_weight_decay, skip_nonfinite, ema_decay, device_state, or a one-element fp32 device
    tensor as `lr` (read by the step's own launch: a schedule writes it, no host value is needed) moves the step's scalar state
    -- step number, bias corrections, clip coefficient, the decision to apply or skip -- into a 64-byte block on the device
    (twog_optim_state_t) that one small launch advances (twog_optim_prepare) in front of the element-wise update
    (twog_optim_apply); without them the launches are exactly the ones above. The arithmetic is stated in include/twog_gcn.h:
    one fp32 rounding per operation, the bias corrections from fp64 running products of the betas (tests/optim_state_ref.py
    reproduces it bit for bit); it differs from the path above by contraction and the form of the bias corrections only.
      decoupled_weight_decay: AdamW, p <- p (1 - lr weight_decay) in front of the update instead of L2 added to the gradient.
      skip_nonfinite: the norm of the model's gradients and, with extra modules, a second norm over theirs are taken; if either
        is not finite the step is SKIPPED on the device: parameters, moments, averaged weights, step number and powers stay
        as they are and skipped_steps() counts it. The norm is an fp32 number: one that is not representable in fp32 (beyond
        3.4e38, from finite gradients) counts as non-finite. Under DataParallel every rank sees the same all-reduced gradient
        and therefore takes the same decision.
      ema_decay: averaged weights ema <- d ema + (1 - d) p' inside the update (they start as a copy of the parameters);
        ema_state_dict() / swap_ema() give them to an evaluation.
    step() returns the pre-clip norm of the model's gradients whenever one was computed and reads nothing on the host.
    Out of scope: learning rates or decay per group, amsgrad, capture of the step into a hipGraph."""

    def __init__(self, flat: FlatParameters, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0,
                 decoupled_weight_decay=False, skip_nonfinite=False, ema_decay=None, device_state=False):
        if not max_grad_norm >= 0.0:
            raise ValueError(f'max_grad_norm must be >= 0, got {max_grad_norm}')
        if ema_decay is not None and not 0.0 < ema_decay < 1.0:
            raise ValueError(f'ema_decay must lie in (0, 1), got {ema_decay}')
        if torch.is_tensor(lr) and not (lr.dtype == torch.float32 and lr.numel() == 1 and lr.device == flat.flat.device):
            raise ValueError('a tensor lr must be one fp32 element on the device of the parameters')
        self.flat, self.lr, self.betas, self.eps, self.wd = flat, lr, betas, eps, weight_decay
        self.max_grad_norm = float(max_grad_norm)
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self.step_count = 0   # the path without device state; step_number() answers on both
        self.decoupled, self.skip_nonfinite = bool(decoupled_weight_decay), bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.on_device = bool(self.decoupled or self.skip_nonfinite or ema_decay is not None or device_state
                              or torch.is_tensor(lr))
        self.ema = flat.flat.detach().clone() if ema_decay is not None else None
        self.state = get_kernels().new_optim_state(0, 0, betas[0], betas[1], flat.flat.device) if self.on_device else None
        self._skipped, self._swapped = 0, False

    def step(self, grad_scale=1.0):
        if self._swapped:
            raise RuntimeError('step() inside swap_ema(): the parameter buffer holds the averaged weights')
        if self.on_device:
            return self._device_step(grad_scale)
        self.step_count += 1
        K, f = get_kernels(), self.flat
        args = (self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.step_count, grad_scale)
        if not self.max_grad_norm:
            K.adam_step(f.flat, f.grad, self.exp_avg, self.exp_avg_sq, *args)
            return None
        b, e = f.module_ranges[0]
        out = K.grad_norm(f.grad, [(b, e)], grad_scale, self.max_grad_norm)
        K.adam_step_coef(f.flat[b:e], f.grad[b:e], self.exp_avg[b:e], self.exp_avg_sq[b:e], *args, out[1:2])
        if e < f.numel:   # the extra modules: never clipped
            K.adam_step(f.flat[e:], f.grad[e:], self.exp_avg[e:], self.exp_avg_sq[e:], *args)
        return out[0]

    def _hyper(self, grad_scale=1.0):
        return dict(beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.wd, grad_scale=grad_scale,
                    ema_decay=self.ema_decay)

    def _device_step(self, grad_scale):
        """Norm(s), one prepare launch, one update launch per range; nothing is read on the host."""
        K, f = get_kernels(), self.flat
        b, e = f.module_ranges[0]
        hyper, clip = self._hyper(grad_scale), self.max_grad_norm > 0
        norms, out = [], None
        if clip or self.skip_nonfinite:
            out = K.grad_norm(f.grad, [(b, e)], grad_scale, self.max_grad_norm)
            norms.append(out[0:1])
            if self.skip_nonfinite and e < f.numel:
                norms.append(K.grad_norm(f.grad, [(e, f.numel)], grad_scale, 0.0)[0:1])
        flags = (K.OPTIM_DECOUPLED if self.decoupled else 0) | (K.OPTIM_SKIP_NONFINITE if self.skip_nonfinite else 0)
        K.optim_prepare(self.state, hyper, self.lr, norms=norms, coef=out[1:2] if clip else None, flags=flags)
        ema = self.ema
        K.optim_apply(f.flat[b:e], f.grad[b:e], self.exp_avg[b:e], self.exp_avg_sq[b:e], None if ema is None else ema[b:e],
                      hyper, flags | (K.OPTIM_CLIP if clip else 0), self.state)
        if e < f.numel:   # the extra modules: never clipped
            K.optim_apply(f.flat[e:], f.grad[e:], self.exp_avg[e:], self.exp_avg_sq[e:], None if ema is None else ema[e:],
                          hyper, flags, self.state)
        return None if out is None else out[0]

    # ---------------------------------------------------------------- step state and checkpoints
    def _read_state(self):
        """(step, skipped, beta1^step, beta2^step): one device-to-host copy on the device path, host values otherwise (the
        powers then by `step` fp64 multiplications, the form the device keeps)."""
        from .kernels import optim_state_block, read_optim_state
        if self.on_device:
            s = read_optim_state(self.state)
        else:
            s = read_optim_state(optim_state_block(self.step_count, self._skipped, *self.betas))
        return s['step'], s['skipped'], s['beta1_pow'], s['beta2_pow']

    def step_number(self):
        """Applied steps so far (one device-to-host copy on the device path)."""
        return self._read_state()[0]

    def skipped_steps(self):
        """Steps skipped for a non-finite gradient norm so far (one device-to-host copy on the device path)."""
        return self._read_state()[1]

    def _view(self, buf, p):
        off = p.data.storage_offset()   # the parameter is a view into flat.flat; every buffer here has its layout
        return buf[off:off + p.numel()].view_as(p)

    def state_dict(self):
        """torch.optim.Adam's layout: group 0 = the model's parameters in model.parameters() order, one further group per extra
        module (how the reference adds the loss learner, train.py:46); per parameter `step`, `exp_avg`, `exp_avg_sq` (copies).
        torch.optim.Adam(model.parameters(), ...) [+ add_param_group per extra module] loads it and this class loads Adam's.
        Our own extras sit under the top-level key 'twog' (torch ignores it): the exact step, the skipped steps, the two fp64
        powers and, with ema_decay, the averaged weights per parameter."""
        step, skipped, p1, p2 = self._read_state()
        lr = float(self.lr.detach().cpu()) if torch.is_tensor(self.lr) else self.lr
        state, groups, ema, i = {}, [], {}, 0
        for g in self.flat.named_groups:
            ids = []
            for _name, p in g:
                state[i] = dict(step=torch.tensor(float(step)), exp_avg=self._view(self.exp_avg, p).detach().clone(),
                                exp_avg_sq=self._view(self.exp_avg_sq, p).detach().clone())
                if self.ema is not None:
                    ema[i] = self._view(self.ema, p).detach().clone()
                ids.append(i)
                i += 1
            groups.append(dict(lr=lr, betas=tuple(self.betas), eps=self.eps, weight_decay=self.wd, amsgrad=False, maximize=False,
                               foreach=None, capturable=False, differentiable=False, fused=None,
                               decoupled_weight_decay=self.decoupled, params=ids))
        twog = dict(step=int(step), skipped=int(skipped), beta1_pow=p1, beta2_pow=p2)
        if self.ema is not None:
            twog['ema'] = ema
        return dict(state=state, param_groups=groups, twog=twog)

    def load_state_dict(self, sd):
        """Loads state_dict()'s result or a torch.optim.Adam state of the same parameters in the same groups. lr, betas, eps and
        weight_decay come from the checkpoint (equal in every group: per-group values are out of scope). A state without 'twog'
        (torch's own) gives skipped = 0 and powers rebuilt by `step` fp64 multiplications; parameters torch kept no state for
        (never given a gradient) get zero moments. Averaged weights are taken when both sides have them; otherwise they stay."""
        groups, named = sd['param_groups'], self.flat.named_groups
        if [len(g['params']) for g in groups] != [len(g) for g in named]:
            raise ValueError(f'the checkpoint has parameter groups of {[len(g["params"]) for g in groups]} parameters, this '
                             f'optimizer {[len(g) for g in named]}')
        keys = ('lr', 'betas', 'eps', 'weight_decay')
        if any(tuple(g[k]) != tuple(groups[0][k]) if k == 'betas' else g[k] != groups[0][k] for g in groups for k in keys):
            raise ValueError('learning rate, betas, eps or weight decay differ between the groups: out of scope here')
        if any(g.get('amsgrad') or g.get('maximize') for g in groups):
            raise ValueError('amsgrad / maximize are out of scope here')
        if bool(groups[0].get('decoupled_weight_decay', False)) != self.decoupled:
            raise ValueError('decoupled_weight_decay of the checkpoint and of this optimizer differ')
        twog, steps = sd.get('twog'), set()
        with torch.no_grad():
            for g_sd, g in zip(groups, named):
                for i, (_name, p) in zip(g_sd['params'], g):
                    st = sd['state'].get(i)
                    for key, buf in (('exp_avg', self.exp_avg), ('exp_avg_sq', self.exp_avg_sq)):
                        if st is None:
                            self._view(buf, p).zero_()
                        else:
                            self._view(buf, p).copy_(st[key])
                    if st is not None:
                        steps.add(int(st['step']))
                    if self.ema is not None and twog is not None and 'ema' in twog:
                        self._view(self.ema, p).copy_(twog['ema'][i])
            lr = float(groups[0]['lr'])
            if torch.is_tensor(self.lr):
                self.lr.fill_(lr)
            else:
                self.lr = lr
        if len(steps) > 1:
            raise ValueError(f'the parameters of the checkpoint are at different steps {sorted(steps)}: out of scope here')
        self.betas, self.eps, self.wd = tuple(groups[0]['betas']), groups[0]['eps'], groups[0]['weight_decay']
        step = twog['step'] if twog is not None else (steps.pop() if steps else 0)
        powers = (twog['beta1_pow'], twog['beta2_pow']) if twog is not None else None
        self.step_count, self._skipped = int(step), int(twog['skipped']) if twog is not None else 0
        if self.on_device:
            self.state = get_kernels().new_optim_state(self.step_count, self._skipped, self.betas[0], self.betas[1],
                                                       self.flat.flat.device, powers=powers)

    # ---------------------------------------------------------------- averaged weights
    def ema_state_dict(self):
        """name -> averaged weights (copies) of the model's parameters, for model.load_state_dict(..., strict=False). BatchNorm
        statistics are buffers, not parameters: they are not averaged."""
        if self.ema is None:
            raise RuntimeError('no averaged weights: construct with ema_decay')
        return {name: self._view(self.ema, p).detach().clone() for name, p in self.flat.named_groups[0]}

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside the context the parameter buffer holds the averaged weights and the EMA buffer the parameters (exchanged with
        the library's copy launches through a temporary), so that an evaluation runs on the averaged weights in place; leaving
        it exchanges them back, bit for bit. step() inside raises."""
        if self.ema is None:
            raise RuntimeError('no averaged weights: construct with ema_decay')
        if self._swapped:
            raise RuntimeError('swap_ema() is already active')
        self._exchange()
        self._swapped = True
        try:
            yield self
        finally:
            self._exchange()
            self._swapped = False

    def _exchange(self):
        K, a, b = get_kernels(), self.flat.flat, self.ema
        tmp = torch.empty_like(a)
        for src, dst in ((a, tmp), (b, a), (tmp, b)):   # three launches: each reads what the one before wrote
            K.copy_blocks([(src, dst)])


def _ranks_share_a_device(group, world):
    """True if two ranks of the group run on the same physical GPU (host name + PCI address of the current device,
    gathered over the group; a collective -- every rank constructs its wrapper)."""
    import socket
    ident = [socket.gethostname()]
    try:
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        ident += [str(getattr(pr, 'uuid', '')), getattr(pr, 'pci_domain_id', -1), getattr(pr, 'pci_bus_id', -1),
                  getattr(pr, 'pci_device_id', -1)]
        if ident[1:] == ['', -1, -1, -1]:   # no hardware identity on this torch build: visible ordinal + visibility mask
            ident += [torch.cuda.current_device(), os.environ.get('HIP_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))]
    except Exception:   # noqa: BLE001 -- identity is best effort; unknown means "assume shared" only if ordinals collide
        ident += [torch.cuda.current_device(), os.environ.get('HIP_VISIBLE_DEVICES', os.environ.get('CUDA_VISIBLE_DEVICES', ''))]
    seen = [None] * world
    dist.all_gather_object(seen, tuple(ident), group=group)
    return len(set(seen)) < world


class DataParallel:
    """model + flat buffers + gradient all-reduce. Usage per step:
        dp.zero_grad(); loss = f(dp.model(...)); loss.backward(); dp.all_reduce_gradients(); opt.step(dp.grad_scale)"""

    def __init__(self, model: torch.nn.Module, process_group=None, bucket_mb: int = 64, broadcast: bool = True,
                 sync_bn: bool = False, global_noise_seed: int = None, overlap: bool = True,
                 count_weighted_loss: bool = False, force_collectives: bool = False, extra_modules=(),
                 device_noise_seed: int = None):
        """sync_bn: the geometric-level BatchNorm uses the statistics of the GLOBAL batch (one all-reduce of 2*4N fp64
        sums per step). count_weighted_loss: every term of the criterion (losses.multi_task_loss) is
        normalised by the GLOBAL number of valid (non-ignored) targets instead of the rank's own (one all-reduce of the
        6-12 per-term counts per step, 8-16 with the temporal smoothing terms, whose pair counts ride in the same tensor;
        8e (b)) -- with ragged clips (-1 targets) the averaged rank gradients are then the
        gradient of the global mean, not a mean of per-rank means. global_noise_seed: every rank draws the Gumbel noise of
        the global batch from a generator seeded with this value and keeps its shard (8e (c)); device_noise_seed gives the
        same equivalence without the W-fold host draw: the noise is drawn on the device (model.use_device_noise(seed)) as a
        function of (seed, forward number, GLOBAL clip index rank * bs + b, time step, entity), so every rank draws its own
        clips only. The two are mutually exclusive. With all three (and equal
        shard sizes) W ranks compute what one process computes on the whole batch; the throughput default keeps them off
        (standard DDP semantics; equal-length synthetic clips make the counts equal anyway).
        force_collectives: run every collective (broadcast, stage-hooked asynchronous all-reduces, count / statistics
        reductions) even in a process group of ONE rank, where they are identities -- lets a single-GPU box execute the
        RCCL path itself (tests/test_distributed_gpu.py).
        extra_modules: modules trained beside the model (the multi-task loss learner, multi_task.MultiTaskLossLearner):
        their parameters live in the same flat buffers after the model's, are broadcast and all-reduced with them and
        stepped by the same FusedAdam (the reference's optimizer.add_param_group, train.py:42-46); FusedAdam's clipping
        leaves them out."""
        if global_noise_seed is not None and device_noise_seed is not None:
            raise ValueError('global_noise_seed and device_noise_seed are two routes to the same noise: pass one of them')
        self.model = model
        self.extra_modules = list(extra_modules)
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        if force_collectives and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError('force_collectives needs an initialised process group')
        self.collective = self.world > 1 or bool(force_collectives)
        if self.world > 1 and torch.cuda.is_available() and _ranks_share_a_device(process_group, self.world):
            # several ranks on one device (a test rig, not a deployment): no launch may assume it owns every compute unit
            from . import kernels as _kernels
            _kernels.PERSIST.shared_devices.add(torch.cuda.current_device())   # per device, not per process
        rank = dist.get_rank(process_group) if self.collective else 0
        self._works, self._launched = [], set()
        self._markers, self._late_failure = [], None
        self.collective_calls = 0   # collectives issued so far (tests assert the path really ran)
        from . import ops
        # Everything this wrapper hangs beside the model (ops.set_model_extra: a weak-KEYED table) refers back to the wrapper
        # only WEAKLY -- the wrapper holds the model, so a strong reference from a table value would keep the weak key, the
        # model and the flat parameter / gradient buffers alive for the life of the process (a discarded wrapper in a sweep
        # loop, an EMA re-wrap). A dead wrapper's callables are no-ops.
        me_ref = weakref.ref(self)
        self._installed = {}   # key -> the object THIS wrapper put into the model's side table (none refers to the wrapper)
        if sync_bn:
            def reduce_stats(sums, n_frames, world=self.world, group=process_group, on=self.collective, me_ref=me_ref):
                if on:
                    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
                    me = me_ref()
                    if me is not None:
                        me.collective_calls += 1
                return sums, n_frames * world
            ops.set_model_extra(model, 'bn_stats_reduce', reduce_stats)
            self._installed['bn_stats_reduce'] = reduce_stats
        self._count_reducer = None
        if count_weighted_loss:
            def reduce_counts(counts, world=self.world, group=process_group, on=self.collective, me_ref=me_ref):
                """counts: fp64 [terms] valid targets of this rank -> global count / W (the rank losses are averaged)."""
                if on:
                    dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
                    me = me_ref()
                    if me is not None:
                        me.collective_calls += 1
                return counts / world
            self._count_reducer = reduce_counts
        if global_noise_seed is not None:
            shard = (rank, self.world, torch.Generator().manual_seed(int(global_noise_seed)))
            ops.set_model_extra(model, 'noise_shard', shard)
            self._installed['noise_shard'] = shard
        if device_noise_seed is not None:
            model.use_device_noise(device_noise_seed)
            noise = ops.get_model_extra(model, 'device_noise')
            noise['rank'] = rank   # clip b of this rank's batch is clip rank * bs + b of the global batch (equal shard sizes)
            self._installed['device_noise'] = noise
        # gradients are laid out in the order the backward pass finishes them (ops.grad_ready_stage), so that each
        # stage's all-reduce can start from inside the backward pass and overlap with the rest of it
        self.flat = FlatParameters(model, stage_of=ops.grad_ready_stage if overlap else None,
                                   extra_modules=self.extra_modules)
        self.bucket = max(1, bucket_mb) * (1 << 20) // 4
        if overlap and self.collective:
            # scoped to this model; close() removes it. A WeakMethod: the table must not own the wrapper (see above)
            ops.set_grad_stage_hook(model, weakref.WeakMethod(self._stage_ready))
        weakref.finalize(self, _drop_extras, weakref.ref(model), me_ref, self._installed)
        if self.collective and broadcast:
            dist.broadcast(self.flat.flat, src=0, group=self.group)
            for m in [model] + self.extra_modules:
                for b in m.buffers():
                    dist.broadcast(b, src=0, group=self.group)
            self.collective_calls += 1

    def close(self):
        """Detaches this wrapper from the model (stage hook, sync-BN / noise-shard / device-noise / loss-count settings: the
        model draws its noise on the host again). Also available as remove()."""
        from . import ops
        hook = ops.get_model_extra(self.model, 'stage_hook')
        if isinstance(hook, weakref.WeakMethod) and hook() == self._stage_ready:
            ops.set_grad_stage_hook(self.model, None)
        _remove_installed(self.model, self._installed)
        self._count_reducer = None

    remove = close

    def loss_scope(self):
        """Context manager for the criterion call(s) of ONE training step: inside it, with count_weighted_loss=True, every
        term of losses.multi_task_loss is normalised by the GLOBAL number of valid targets (one all-reduce of the per-term
        counts per criterion call). The reduction is a collective: every rank must enter the scope and call the criterion
        the same number of times inside it. Outside the scope -- validation on one rank, a second model, no_grad
        evaluation -- the criterion is the reference's single-process arithmetic and issues no collective.
            with dp.loss_scope():
                loss = sum(criterion(out, targets))"""
        from . import losses
        return losses.count_reducer_scope(self._count_reducer)

    @property
    def grad_scale(self):
        return 1.0 / self.world

    def zero_grad(self):
        self.flat.zero_grad()
        self._works, self._launched = [], set()
        self._markers, self._late_failure = [], None

    def _reduce_range(self, begin, end):
        g = self.flat.grad
        for off in range(begin, end, self.bucket):
            self._works.append(dist.all_reduce(g[off:min(off + self.bucket, end)], op=dist.ReduceOp.SUM,
                                               group=self.group, async_op=True))
            self.collective_calls += 1

    def _stage_ready(self, stage):
        """Called from inside this model's backward pass (ops.set_grad_stage_hook): every gradient of `stage` is final, start its
        all-reduce now (a few large chunks; ring collectives over xGMI are per-link bound)."""
        if stage in self._launched or stage not in self.flat.stage_ranges:
            return
        self._launched.add(stage)
        self._poison_if_a_persistent_launch_gave_up(self.flat.stage_ranges[stage][0])
        self._reduce_range(*self.flat.stage_ranges[stage])

    def _poison_if_a_persistent_launch_gave_up(self, begin):
        """A persistent launch of this rank's backward pass that could not keep its grid resident leaves incomplete
        gradients behind, and its error word is only read at the end of the pass (kernels.py: reading it at once costs
        ~1.2 ms per 8-clip step). The all-reduce about to be issued would spread those gradients to every rank:
        so ONE small launch in front of it (twog_guard_outputs, on the stream the all-reduce is ordered behind) turns the
        first element of this stage's range into NaN if a pending word is set. The sum carries the NaN to every rank, and
        all_reduce_gradients() raises on ALL of them before any optimizer sees the buffer."""
        K = get_kernels()
        if not hasattr(K, 'guard_persistent'):
            return
        marker = self.flat.grad[begin:begin + 1]
        if not K.guard_persistent(self.flat.grad.device, [marker]):
            # (too many pending words for one guard launch, or the guard is switched off: read the words now -- a wait --
            # and poison from the host; never raise in front of a collective the other ranks are entering)
            try:
                K.verify_persistent(self.flat.grad.device)
            except RuntimeError as e:
                self._late_failure = e
                marker.fill_(float('nan'))
        self._markers.append(begin)

    def all_reduce_gradients(self):
        """Sum-all-reduce of the flat gradient buffer: whatever the backward pass has not started yet is launched here
        (a few large chunks, back to back), then everything is waited for. One backward pass per call to zero_grad()."""
        if not self.collective:
            return
        if self.flat.stage_ranges:
            for stage in sorted(self.flat.stage_ranges):
                self._stage_ready(stage)
        else:
            self._reduce_range(0, self.flat.grad.numel())
        for w in self._works:
            w.wait()
        self._works = []
        self._raise_if_any_rank_failed()

    def _raise_if_any_rank_failed(self):
        """After the collectives: this rank's deferred error words (kernels.verify_persistent) and the NaN markers of every
        rank (see _poison_if_a_persistent_launch_gave_up). Raises on every rank alike; the step is to be repeated."""
        K = get_kernels()
        mine = self._late_failure
        self._late_failure = None
        if hasattr(K, 'verify_persistent'):
            try:
                K.verify_persistent(self.flat.grad.device)
            except RuntimeError as e:
                mine = e
        markers, self._markers = self._markers, []
        poisoned = False
        if markers:
            vals = torch.stack([self.flat.grad[b] for b in markers]).cpu()
            poisoned = not bool(torch.isfinite(vals).all())
        if mine is not None and not poisoned and self.world > 1:
            # (a failure the guard launch did not see -- the word landed after it ran: cannot happen with the words ordered
            # on the stream in front of the guard, but the other ranks must not step on what this rank knows is incomplete)
            self.flat.grad.fill_(float('nan'))
        if mine is not None:
            raise mine
        if poisoned:
            raise RuntimeError('a rank of this group could not complete a persistent launch of its backward pass (or produced '
                               'a non-finite gradient): the all-reduced gradient buffer is marked NaN on every rank and must '
                               'not reach the optimizer. Repeat the step (zero_grad, forward, backward).')

    def shard(self, tensor, rank=None):
        """This rank's contiguous slice [r*bs/W, (r+1)*bs/W) of a global batch."""
        rank = dist.get_rank(self.group) if rank is None and self.collective else (rank or 0)
        n = tensor.shape[0] // self.world
        return tensor[rank * n:(rank + 1) * n]
