"""torch tensors (and anything that speaks DLPack) as the data argument of `fit` / `dp_parallel` / `resume_from_checkpoint` / `predict`:
recognise the input and describe it, as host/sparse.py does for sparse columns.  torch is imported lazily -- the package imports without it.

Shape is Dimensions x Samples, as everywhere.  Accepted element types: float16, bfloat16, float32, float64, uint8, int16, int32, int64; any
strides (a transposed view, a column range, steps, `expand`).  An (N, D) tensor of embeddings comes in as `emb.T`: a view, no copy -- the
device then reads it with the features contiguous, its fast case.

  * a tensor on a ROCm device is described by a `DeviceTensor` (pointer, element type, the two strides): the worker reads it in place
    (include/dpmm_hip_tensor.h) and labels / predictions come back as tensors on that device;
  * a tensor on the CPU becomes a numpy array and takes the existing host path: a zero-copy view where numpy has the element type,
    through `.float()` otherwise (bfloat16).
"""
import sys

import numpy as np

DT_F16, DT_BF16, DT_F32, DT_F64, DT_U8, DT_I16, DT_I32, DT_I64 = range(8)      # DPMM_DT_* of include/dpmm_hip_tensor.h
_DTYPE_NAMES = ("float16", "bfloat16", "float32", "float64", "uint8", "int16", "int32", "int64")
ITEMSIZE = (2, 2, 4, 8, 1, 2, 4, 8)


def _torch():
    """torch if the caller has imported it (a tensor cannot exist otherwise), else None: recognising an array must not import torch."""
    return sys.modules.get("torch")


def _dtype_code(torch, dtype):
    for code, name in enumerate(_DTYPE_NAMES):
        if dtype == getattr(torch, name):
            return code
    raise TypeError(f"tensor data of dtype {dtype} is not supported: one of {', '.join(_DTYPE_NAMES)}")


class DeviceTensor:
    """A (D, N) tensor in device memory: element (feature d, point i) at data_ptr + (i * stride_point + d * stride_feature) * itemsize."""

    def __init__(self, tensor, dtype):
        self.tensor = tensor                       # keeps the memory alive for as long as the description is
        self.shape = (int(tensor.shape[0]), int(tensor.shape[1]))
        self.D, self.N = self.shape
        self.dtype = dtype
        self.itemsize = ITEMSIZE[dtype]
        self.stride_feature, self.stride_point = (int(v) for v in tensor.stride())
        self.data_ptr = int(tensor.data_ptr())
        self.torch_device = tensor.device
        self.device_index = tensor.device.index if tensor.device.index is not None else 0

    def shard_ptr(self, lo):
        """Address of point `lo`'s first feature: the points [lo, hi) are the same description from there."""
        return self.data_ptr + int(lo) * self.stride_point * self.itemsize

    def synchronize(self):
        """The tensor's values must be complete before the library reads them on its own stream."""
        import torch
        torch.cuda.current_stream(self.torch_device).synchronize()


def _check(torch, t):
    if t.layout != torch.strided:
        raise TypeError(f"tensor data must be dense (strided); got layout {t.layout} -- sparse count data comes in as scipy CSC, a tuple or a torch.sparse_csc tensor (tensor.to_sparse_csc())")
    if t.is_quantized:
        raise TypeError(f"tensor data of dtype {t.dtype} (quantised) is not supported")
    code = _dtype_code(torch, t.dtype)
    if t.requires_grad:
        raise TypeError("tensor data requires grad: pass tensor.detach()")
    if t.ndim != 2:
        raise TypeError(f"tensor data must be 2-D, Dimensions x Samples; got {t.ndim}-D")
    return code


def is_tensor(data):
    torch = _torch()
    return torch is not None and isinstance(data, torch.Tensor)


def as_tensor(data):
    """The torch tensor behind `data` (a tensor, or a non-numpy object offering __dlpack__), or None for everything else."""
    if is_tensor(data):
        return data
    if hasattr(data, "__dlpack__") and not isinstance(data, np.ndarray):
        import torch
        return torch.from_dlpack(data)
    return None


def describe(tensor):
    """DeviceTensor of a tensor that can be taken, wherever it lives (raises TypeError otherwise)."""
    return DeviceTensor(tensor, _check(sys.modules["torch"], tensor))


def as_device_points(all_data):
    """DeviceTensor for a tensor in device memory; None for everything that is handled otherwise (arrays, sparse input, CPU tensors).
    Raises TypeError for a tensor that cannot be taken (element type, layout, requires_grad, ndim)."""
    t = as_tensor(all_data)
    if t is None:
        return None
    desc = describe(t)
    if t.device.type == "cpu":
        return None
    if t.device.type != "cuda":
        raise TypeError(f"tensor data lives on device {t.device}: a ROCm device or the CPU is needed")
    return desc


def as_host_array(all_data):
    """`all_data` with a CPU tensor replaced by a numpy array of the same values (a view where numpy has the element type, `.float()` for
    bfloat16); everything else is returned as it came."""
    t = as_tensor(all_data)
    if t is None or t.device.type != "cpu":
        return all_data
    code = _check(sys.modules["torch"], t)
    return t.float().numpy() if code == DT_BF16 else t.numpy()


def host_int64(values):
    """Ground-truth labels and the like: a tensor (any device) comes to the host as int64; anything else is returned as it came."""
    if is_tensor(values):
        return values.detach().to("cpu").to(sys.modules["torch"].int64).numpy()
    return values


def resolve_device(desc, device):
    """The device index a worker for `desc` is created on: the tensor's; an explicit `device` must agree."""
    if device is not None:
        if isinstance(device, str):
            device = sys.modules["torch"].device(device)
        idx = device if isinstance(device, (int, np.integer)) else device.index      # (torch.device("cuda").index is None: the current one)
        if idx is not None and int(idx) != desc.device_index:
            raise ValueError(f"device={device!r} disagrees with the data tensor's device {desc.torch_device}")
    return desc.device_index
