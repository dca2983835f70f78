"""What the row-pass wrappers (metrics.trajectory_metrics, constrain.score_rows / resample, diagnose.forcing_rows,
pulse.pulse_response, joint) share between their own checks and their own C call: the `steps` of the rows, the device-row
check, the rule by which a view is walked in place or copied, the shared tables of the two forcing passes, the weights and the
mask of a summary, and the call through the C ABI.  Plain functions; every wrapper names its own entry point and keeps the
messages that are its own.
"""
import ctypes

import numpy as np
import torch


def model_steps(steps, K, *, increasing=True, non_negative=False, n_steps=None):
    """`steps` as int64 [K]: the model step each of K rows holds.  increasing: strictly (False where the caller asks for
    consecutive steps itself, diagnose.check_consecutive).  non_negative: the steps lie in 0..2^31-1 — for a pass without a
    table that bounds them.  n_steps: the tables' steps, checked by steps_in_tables."""
    st = np.asarray(steps)
    if st.shape != (K,) or (K and not np.issubdtype(st.dtype, np.integer)):
        raise ValueError(f"steps: want {K} integers, one per row")
    st = st.astype(np.int64)
    if K and ((non_negative and (st[0] < 0 or st[-1] >= 2 ** 31)) or (increasing and np.any(np.diff(st) <= 0))):
        raise ValueError(f"steps: want {'non-negative, ' if non_negative else ''}strictly increasing model steps")
    if n_steps is not None:
        steps_in_tables(st, n_steps)
    return st


def steps_in_tables(st, n_steps):
    """ValueError unless the increasing steps `st` lie inside tables of n_steps steps (a wrapper that builds its tables after
    the other checks on `steps` calls this on its own)."""
    if st.size and (st[0] < 0 or st[-1] >= n_steps):
        raise ValueError(f"steps: {int(st[0])}..{int(st[-1])} outside the tables' steps 0..{n_steps - 1}")


def steps_i32(st, dev):
    return torch.from_numpy(st.astype(np.int32)).to(dev)


def dev_rows(t, shape, name, dtype, dev):
    """`t` if it is a `dtype` tensor of `shape` on the GPU `dev`; ValueError / TypeError naming it otherwise."""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype:
        raise ValueError(f"{name}: want a {dtype} tensor of shape {list(shape)}")
    if not t.is_cuda:
        raise TypeError(f"{name} must be on the GPU (got {t.device}): there is no CPU path")
    if t.device != dev:
        raise ValueError(f"{name}: on {t.device}, the rows on {dev}")
    return t


def walk_in_place(x, N, *, first=0, always=(), copy=False):
    """x [..., N], the last axis the members: (x or its contiguous copy, the strides of the leading axes as the C ABI takes
    them).  A kernel walks the view in place when the member stride is 1 (not examined for N = 1) and every leading axis of
    extent > 1 lies at least N apart (a stride of 0 — an expanded view — does not); an axis of extent 1 reports N whatever
    the view says.  (torch has no negative strides, so no magnitude is taken.)
    first: the first leading axis under the rule — those before it are the caller's to judge and are not reported.
    always: axes examined and reported as they lie even at extent 1.  copy: the caller's own reason to copy."""
    axes = range(first, x.dim() - 1)
    live = [a in always or x.shape[a] > 1 for a in axes]
    if copy or (N > 1 and x.stride(-1) != 1) or any(l and x.stride(a) < N for a, l in zip(axes, live)):
        x = x.contiguous()
    return x, tuple(int(x.stride(a)) if l else N for a, l in zip(axes, live))


def drive_table(F_ext, lead, name, dtype, dev):
    """The drive table(s) `lead` + [n_steps, DRIVE_STRIDE] on `dev`: a device table of that rank taken as it is (`name` in its
    refusals), else the external forcing as host values — [n_steps], with lead = (S,) also [S, n_steps] — in column 6 of a
    zero table."""
    from ._capi import DRIVE_STRIDE
    if isinstance(F_ext, torch.Tensor) and F_ext.dim() == len(lead) + 2:
        return dev_rows(F_ext, lead + (int(F_ext.shape[-2]), DRIVE_STRIDE), name, dtype, dev).contiguous()
    fe = np.asarray(F_ext.cpu() if isinstance(F_ext, torch.Tensor) else F_ext, dtype=np.float64)
    if not lead:
        fe = fe.reshape(-1)
    else:
        fe = np.broadcast_to(fe, lead + fe.shape[-1:]) if fe.ndim == 1 else fe
        if fe.ndim != 2 or fe.shape[0] != lead[0]:
            raise ValueError(f"F_ext: want [n_steps] or [{lead[0]}, n_steps]")
    table = np.zeros(fe.shape + (DRIVE_STRIDE,))
    table[..., 6] = fe
    return torch.from_numpy(table).to(dev, dtype)


def forcing_tables(fscale, X, lead, G, N, n_steps, dtype, dev, *, together, x_name, host_table):
    """(n_fext, fext, fscale) of a forcing= run: the categories K, their table `lead` + [n_steps, MAX_FEXT] on `dev` and the
    checked scale rows [G + K, N]; (0, None, None) for a plain run.  X on the device is taken as it is (`x_name` in its
    refusals) and K = fscale's rows - G; any other X goes through host_table(X), the caller's table class with its own refusal
    of a table of other extents.  together: the refusal of one of fscale / X without the other."""
    from ._capi import MAX_FEXT
    if (fscale is None) != (X is None):
        raise ValueError(together)
    if fscale is None:
        return 0, None, None
    if isinstance(X, torch.Tensor):
        n_fext = int(fscale.shape[0]) - G
        fext = dev_rows(X, lead + (n_steps, MAX_FEXT), x_name, dtype, dev).contiguous()
    else:
        fx = host_table(X)
        n_fext = fx.n_categories
        fext = torch.from_numpy(fx.padded()).to(dev, dtype)
    if not 0 <= n_fext <= MAX_FEXT:
        raise ValueError(f"fscale: {int(fscale.shape[0])} rows for {G} gases: want G + K rows, K <= {MAX_FEXT}")
    return n_fext, fext, dev_rows(fscale, (G + n_fext, N), "fscale", dtype, dev)


def ptr(t):
    """The address of tensor `t` as the C ABI takes it; NULL for None."""
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def call(lib, capi, base, dtype, dev, *args, stream=None, guard=None):
    """One call of a C entry point whose last argument is the stream: `base`_f64 / `base`_f32 by the rows' dtype (`base` itself
    for dtype None), on the current stream of `dev` inside its device guard — or, for a wrapper with a _lib_and_stream switch,
    on the `stream` and inside the `guard` that switch handed out.  The return code goes to capi.check."""
    fn = getattr(lib, base if dtype is None else f"{base}_{'f64' if dtype == torch.float64 else 'f32'}")
    with torch.cuda.device(dev) if guard is None else guard:
        if guard is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        capi.check(lib, fn(*args, stream))


def int_weights(weights, n, dev, *, check_range):
    """`weights` if it is an int64 tensor [n] on `dev` (check_range: with every value in 0..2^32, which costs a download)."""
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.int64 or tuple(weights.shape) != (n,) or weights.device != dev:
        raise ValueError(f"weights: want an int64 tensor of shape [{n}] on {dev}")
    if check_range and n and (int(weights.min()) < 0 or int(weights.max()) > (1 << 32)):
        raise ValueError("weights: values outside [0, 2^32]")
    return weights


def bool_mask(accepted, n, dev):
    """`accepted` as a boolean tensor [n] on `dev`."""
    mask = torch.as_tensor(accepted, device=dev)
    if mask.dtype != torch.bool or tuple(mask.shape) != (n,):
        raise ValueError(f"accepted: want a boolean mask of shape [{n}]")
    return mask
