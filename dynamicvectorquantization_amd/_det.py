"""The package's one reproducibility switch (no import of torch or the library until it is asked).

`set_deterministic(None | True | False)`: with the switch ON the per-code sums of the training step -- the EMA statistics and the
codebook gradient -- run on the kernels that add in one fixed order (`dvq_code_sums_det`, `dvq_vq_backward_codebook_det_f32`:
equal inputs give equal bits); OFF they run on the float-atomic kernels, which add in arrival order.  None, the default, follows
`torch.are_deterministic_algorithms_enabled()` at call time.  Outside the switch: the order in which a data-parallel all_reduce
adds the ranks' statistics (the collective library's), and every random draw (torch's generators)."""
import contextlib

_STATE = None


def set_deterministic(flag):
    """None: follow torch.use_deterministic_algorithms; True / False: the package's own choice.  Returns the previous setting."""
    global _STATE
    if flag is not None and not isinstance(flag, bool):
        raise TypeError("set_deterministic takes None, True or False, got %r" % (flag,))
    previous, _STATE = _STATE, flag
    return previous


def is_deterministic(override=None):
    """what a call does now: `override` if given, else the switch, else torch's flag"""
    if override is not None:
        return bool(override)
    if _STATE is not None:
        return _STATE
    import torch
    return torch.are_deterministic_algorithms_enabled()


@contextlib.contextmanager
def torch_deterministic():
    """torch's own flag held on for the torch ops of a fallback path (index_add_ is then order-stable, or raises as torch does).
    The flag is PROCESS-WIDE, so this is not thread-safe: while a fallback runs (CPU tensors, K above the kernels' limit, the
    codebook gradient of 16-bit latents) another thread sees it on and may get torch's error from an op without a deterministic
    form.  A caller with such threads enables torch.use_deterministic_algorithms(True) itself, for the whole process; then
    nothing is flipped here.  The kernel paths never touch the flag."""
    import torch
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    if was and not warn:
        yield
        return
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
