"""The optimizers without a device, for the host tests: a REAL `FlatAdam` on CPU tensors (it needs no library until its first
launch), and a `TrainStep` / `FusedClampAdam` made without `__init__` around one."""
import importlib

sat = importlib.import_module("show-and-tell_amd")
optim = importlib.import_module("show-and-tell_amd.optim")

SLICES = {"w": (0, 6, (2, 3)), "b": (8, 3, (3,))}


def host_flat(slices=SLICES):
    """a FlatAdam over `slices` {name: (offset, numel, shape)} with zeroed CPU buffers, plus the `slices` / `names` TrainStep reads"""
    flat = optim.FlatAdam(list(slices.values()), "cpu")
    flat.slices, flat.names = dict(slices), list(slices)
    return flat


def bare(cls, slices=SLICES):
    """`cls` (TrainStep or FusedClampAdam) without `__init__`, on a host FlatAdam"""
    obj = object.__new__(cls)
    setattr(obj, "flat" if cls is sat.TrainStep else "core", host_flat(slices))
    return obj
