"""Device-side helpers shared by the entry scripts: the pieces of the reference scripts that are
tensor arithmetic (train_generator.py:47-55, 190-194, 245-247, 353-391) routed to the HIP kernels."""
from __future__ import annotations

import torch

from . import ops, trigger

_consts = {}


def _c(hw: int, ratio: float, device):
    key = (hw, ratio, str(device))
    if key not in _consts:
        _consts[key] = (trigger.lowpass_matrix(hw, ratio).to(device), trigger.dct_matrix(hw).float().to(device))
    return _consts[key]


def create_backdoor(netG, inputs: torch.Tensor, opt, sigma: float = None, noise_from: torch.Tensor = None,
                    labels: torch.Tensor = None) -> torch.Tensor:
    """netG -> low_freq -> clamp(x + noise*rate) -> GaussianBlur (one sigma per call, drawn here from
    torch's global generator like T.GaussianBlur) for a float32 NCHW device batch; no gradient.
    noise_from: a batch of the same shape whose generator noise is mixed onto `inputs` instead of their own -- the
    input-aware attack's cross images (train_generator_inputaware.py:236-238, 412-414).
    labels: the classes a label-conditioned generator (nets.CUnetGeneratorv1) poisons the images towards, one per image
    (create_inputs_bd(inputs, targets, netG, opt), train_generator_multilabel.py:67-75); required for it, refused for
    every other generator."""
    n, _, hw, _ = inputs.shape
    if noise_from is not None and tuple(noise_from.shape) != tuple(inputs.shape):
        raise ValueError("create_backdoor: noise_from %s must have the shape of inputs %s"
                         % (tuple(noise_from.shape), tuple(inputs.shape)))
    if (labels is not None) != (netG.arch == "cunet"):
        raise ValueError("create_backdoor: labels are %s" % ("required by a label-conditioned generator" if labels is None
                                                             else "taken by a label-conditioned generator only"))
    if labels is not None:
        from .engine import check_labels
        labels = check_labels(labels, n, netG.num_classes)
    if n == 0:
        return inputs
    eng = netG._net_engine()
    eng.refresh()
    inputs = inputs.contiguous().float()
    if netG.arch == "gridgen":   # WaNet: warp by the generator's field (train_generator_wanet.py:151-157, :346-352)
        if noise_from is not None:
            raise ValueError("create_backdoor: noise_from needs a noise generator (the warping trigger has no per-image noise)")
        from ._lib import lib
        g = eng.forward_grid(hw, float(opt.grid_rescale))
        out = torch.empty_like(inputs)
        ops.check(lib.combat_warp_fwd(inputs.data_ptr(), None, g["grid"].data_ptr(), 0, n, hw, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "combat_warp_fwd")
        return out
    from .engine import pad_batch
    slot = eng.slot("api", pad_batch(n), hw)
    ops.image_to_c8(inputs if noise_from is None else noise_from.contiguous().float(), eng.input(slot))
    if labels is not None:
        eng.labels(slot)[:n].copy_(labels)
    eng.forward_plan(slot).run()
    if sigma is None:
        sigma = trigger.sample_sigma(getattr(opt, "sigma", (0.1, 1.0)))
    pm, _ = _c(hw, opt.ratio, inputs.device)
    k1 = torch.from_numpy(trigger.gaussian_kernel1d(sigma, opt.kernel_size)).to(inputs.device)
    out = torch.empty_like(inputs)
    ops.trigger_fwd(inputs, eng.output(slot), pm, k1, float(opt.noise_rate), out)
    return out


def frequency_logits(netF, inputs_bd: torch.Tensor, opt) -> torch.Tensor:
    """netF(dct_2d(((x + 1) / 2 * 255).byte())) (train_generator.py:245-247, 381-383)."""
    n, _, hw, _ = inputs_bd.shape
    eng = netF._net_engine()
    eng.refresh()
    from .engine import pad_batch
    slot = eng.slot("api", pad_batch(n), hw)
    _, dm = _c(hw, opt.ratio, inputs_bd.device)
    ops.dct_u8(inputs_bd.contiguous().float(), dm, eng.input(slot))
    eng.forward_plan(slot).run()
    return slot.bufs["logits"][:n].clone()


def pooled_features(netC, inputs: torch.Tensor) -> torch.Tensor:
    """The eval-mode classifier's pooled features (the input of its `linear`; preact_resnet.py:99-100, resnet.py:93-95)
    for a float32 NCHW device batch: fp32 [n][in] in torch's NCHW-flatten order, a copy.  It is the pass `netC(inputs)`
    runs -- same slot, same plan, no launch added -- read one buffer earlier (combat_head_fwd's `pooled` output)."""
    if netC.training:
        raise ValueError("pooled_features: the classifier must be in eval mode")
    from .engine import pad_batch
    eng = netC._net_engine()
    eng.refresh()
    n, _, hw, _ = inputs.shape
    slot = eng.slot("module.eval", pad_batch(n), hw)
    ops.image_to_c8(inputs.contiguous().float(), eng.input(slot))
    eng.forward_plan(slot, False).run()
    return eng.head_bufs(slot)["pooled"][:n].clone()


def sync_momentum_to_optimizer(optimizer, module) -> None:
    """The fused SGD keeps momentum in the engine's flat buffer; mirror it into the torch optimiser's
    state so `optimizer.state_dict()` (checkpoint key optimizerC/optimizerG) has the reference layout."""
    eng = module._net_engine()
    for name, p in module.named_parameters():
        optimizer.state[p]["momentum_buffer"] = eng.fp.logical(eng.fp.mom, name).detach().clone()


def load_momentum_from_optimizer(optimizer, module) -> None:
    eng = module._net_engine()
    for name, p in module.named_parameters():
        buf = optimizer.state.get(p, {}).get("momentum_buffer")
        if buf is not None:
            eng.fp.logical(eng.fp.mom, name).copy_(buf)
