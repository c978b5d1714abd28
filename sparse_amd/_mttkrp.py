"""MTTKRP - the matricised tensor times Khatri-Rao product, the inner loop of CP / PARAFAC factorisation - as one fused
kernel (csrc/mttkrp.hip).  The reference has no function for it; its example (examples/mttkrp_example.py) writes

    sparse.sum(B[:, :, :, None] * D[None, None, :, :] * C[None, :, None, :], axis=(1, 2))

which forms two broadcast products of nnz x R stored elements each before it sums them."""
import numpy as np
import torch

from . import _device as dev
from . import _kernels as K
from . import _settings
from ._coo import COO
from ._gcxs import GCXS

_FACTOR_DTYPES = (torch.float32, torch.float64)
_NP_FACTOR = {np.dtype("float32"): torch.float32, np.dtype("float64"): torch.float64}


def mttkrp(x, factors, mode):
    """out[i, r] = sum over the stored elements n of `x` with coords[mode][n] == i of
    data[n] * prod_{d != mode} factors[d][coords[d][n], r].

    `x`: a COO or GCXS of 2 to 8 dimensions with a zero fill value and real, integer or boolean values.  `factors`: a
    sequence of `x.ndim` entries; `factors[d]` is a 2-D `(x.shape[d], R)` NumPy array or torch tensor (host or device, any
    strides), all float32 or all float64 - the result's type, to which the values of `x` are converted on the device;
    `factors[mode]` is ignored and may be None.  `mode`: the kept dimension (negative counts from the end).

    Returns the dense `(x.shape[mode], R)` matrix: a torch device tensor if any factor was a torch tensor, else an ndarray.
    Rows without a stored element are +0.0.  A term is the value times the factors' entries in dimension order, a row is
    summed in stored order (pieces of `_kernels.MTTKRP_CHUNK` elements of a long row are summed on their own and added in
    order): the same bits on every call, no atomics.  The grouping of the stored elements by `coords[mode]` is built once
    per mode and kept on the array (on the COO view of a GCXS)."""
    from ._dot import _validate_derived
    from ._utils import check_zero_fill_value

    if not isinstance(x, (COO, GCXS)):
        raise TypeError(f"mttkrp needs a COO or GCXS tensor, got {type(x).__name__}")
    check_zero_fill_value(x)
    ndim = x.ndim
    if ndim < 2:
        raise ValueError("mttkrp needs a sparse tensor of at least 2 dimensions")
    if ndim > K.MTTKRP_MAX_NDIM:
        raise ValueError(f"mttkrp supports at most {K.MTTKRP_MAX_NDIM} dimensions, got {ndim}")
    if np.dtype(x.dtype).kind not in "fiub":
        raise TypeError(f"mttkrp: tensor values of type {x.dtype} are not supported (real, integer or boolean)")
    if not isinstance(mode, (int, np.integer)) or isinstance(mode, bool):
        raise TypeError("mode must be an integer")
    if not -ndim <= mode < ndim:
        raise ValueError(f"mode {mode} is out of range for a tensor of {ndim} dimensions")
    mode = int(mode) % ndim
    factors = list(factors)
    if len(factors) != ndim:
        raise ValueError(f"shape-mismatch: {len(factors)} factors for a tensor of {ndim} dimensions")
    torch_out = any(isinstance(f, torch.Tensor) for d, f in enumerate(factors) if d != mode)

    if isinstance(x, COO):
        xc = x
    else:  # the COO view of a GCXS operand is kept on it, and the plans on the view (as sddmm does)
        _validate_derived(x)
        xc = x.__dict__.get("_coo_view")
        if xc is None:
            xc = x.__dict__["_coo_view"] = x.tocoo()

    dts, R = set(), None
    for d, f in enumerate(factors):
        if d == mode:
            continue
        if not isinstance(f, (np.ndarray, torch.Tensor)):
            raise TypeError(f"factors[{d}] must be a NumPy array or a torch tensor, got {type(f).__name__}")
        if f.ndim != 2 or int(f.shape[0]) != x.shape[d]:
            raise ValueError(f"shape-mismatch: factors[{d}] has shape {tuple(f.shape)}, expected ({x.shape[d]}, R)")
        if R is None:
            R = int(f.shape[1])
        elif int(f.shape[1]) != R:
            raise ValueError(f"shape-mismatch: factors[{d}] has {int(f.shape[1])} columns, the others {R}")
        dts.add(f.dtype if isinstance(f, torch.Tensor) else _NP_FACTOR.get(f.dtype, f.dtype))
    if len(dts) != 1 or next(iter(dts)) not in _FACTOR_DTYPES:
        raise TypeError("mttkrp: the factors must be all float32 or all float64 (complex and 16-bit factors are not "
                        f"supported), got {sorted(str(t) for t in dts)}")
    dt = next(iter(dts))
    nrows = x.shape[mode]
    if R == 0 or xc.nnz == 0 or nrows == 0:
        out = torch.zeros((nrows, R), dtype=dt, device=xc.device)
        return out if torch_out else dev.to_numpy(out)

    dfac = [None if d == mode else dev.to_device(f, xc.device) for d, f in enumerate(factors)]
    _validate_derived(xc)
    plans = xc.__dict__.setdefault("_mttkrp_plan", {})
    plan = plans.get(mode)
    if plan is None:
        plan = plans[mode] = K.mttkrp_plan(xc.coords, xc.shape, mode)
    data = K.convert(xc.data, dt)
    out = K.mttkrp_coo(xc.coords, data, xc.shape, dfac, mode, plan, exact=_settings.EXACT_MULADD)
    return out if torch_out else dev.to_numpy(out)
