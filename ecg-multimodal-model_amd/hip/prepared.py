"""What every inference plan shares (ecgmm/inference.py, the fused section of ecgmm/tabnet.py): a plan is a *prepared blob*
(the parameters, folded or copied, in the layout its C entry points read) plus a launch on it.

The entry points of a plan are ``prefix + "_infer_prepared_bytes" | "_infer_prepare" | "_infer_workspace" | "_infer"``, with ONE
argument order each, written down once here:
    prepare   (desc, *tables, blob, nbytes, stream)
    run       (desc, *inputs, blob, nbytes, *outputs[, ws, ws_bytes], stream)

A subclass supplies ``prefix`` / ``name`` / ``who``, a ``_desc(*shape)``, a ``refresh()`` that gathers the parameter tables and
assigns ``self.blob = self.prepare(...)`` LAST, and a ``__call__`` that checks its input and returns what ``self.run(...)`` does."""
import ctypes as C

import torch

from . import lib as L
from .encoders import dtype_code
from .functional import _Scratch, _require_cuda, new_bytes, ptr, stream


class PreparedPlan:
    prefix = None        # "ecgmm_resnet18": the C entry points are prefix + "_infer..."
    name = None          # "resnet18": what the library's messages call the plan
    who = None           # "Predictor(resnet18)": what the Python messages call it
    workspace = True     # a run takes a transient workspace (sized by prefix + "_infer_workspace")
    blob = None

    # what Predictor needs to know about a plan
    inputs = ("input",)      # the positional inputs, as the TypeError texts name them
    takes_lengths = False    # called as plan(*inputs, lengths)
    logits = None            # which element of the output is the class logits (None: the output itself)

    def __init__(self, module):
        self.module = module
        self.refresh()

    def batch_args(self, columns):
        """The input columns of one loader batch -> the plan's call arguments (``((input, lengths), labels)`` batches)."""
        if self.takes_lengths and isinstance(columns[0], (tuple, list)):
            return tuple(columns[0])
        return tuple(columns)

    # ---- the two procedures ------------------------------------------------------------------------------------------
    @classmethod
    def _entry(cls, what):
        return getattr(L.lib(), cls.prefix + "_infer" + what)

    @classmethod
    def prepare(cls, desc, tables, device):
        """-> a NEW blob prepared from ``tables`` (lists of tensors): a forward already enqueued with the old one (another
        stream) keeps reading consistent weights, so nothing here ever writes into a blob that was handed out."""
        nb = cls._entry("_prepared_bytes")(C.byref(desc))
        if nb == 0:
            L.check(1, cls.name + " prepared-size query")    # raises the library's message
        with torch.cuda.device(device), torch.no_grad():
            blob = new_bytes(nb, device)
            tables = [(C.c_void_p * len(t))(*[p.data_ptr() for p in t]) for t in tables]
            L.check(cls._entry("_prepare")(C.byref(desc), *tables, ptr(blob), blob.numel(), stream()), cls.name + " infer prepare")
        return blob

    @classmethod
    def workspace_query(cls, desc):
        nb = cls._entry("_workspace")(C.byref(desc))
        if nb == 0:
            L.check(1, cls.name + " infer workspace query")
        return nb

    @classmethod
    def run(cls, desc, blob, inputs, shapes, device):
        """The checked launch on the calling stream -> the outputs, new fp32 tensors of ``shapes`` (None: a null pointer).
        ``inputs``: tensors (None: a null pointer) or ints."""
        arg = lambda t: t if isinstance(t, int) else ptr(t)
        with torch.cuda.device(device):
            tail = ()
            if cls.workspace:
                ws = _Scratch.get(cls.prefix + "_infer", cls.workspace_query(desc), device)   # transient: nothing outlives the call
                tail = (ptr(ws), ws.numel())
            blob.record_stream(torch.cuda.current_stream(device))
            outs = [None if s is None else torch.empty(s, device=device, dtype=torch.float32) for s in shapes]
            L.check(cls._entry("")(C.byref(desc), *map(arg, inputs), ptr(blob), blob.numel(), *map(ptr, outs), *tail, stream()),
                    cls.name + " infer")
        return outs

    def workspace_bytes(self, *shape):
        """Bytes of the inference workspace for an input of ``shape`` (the arguments of the plan's ``_desc``; no GPU work)."""
        return int(self._entry("_workspace")(C.byref(self._desc(*shape))))

    # ---- the two checks ----------------------------------------------------------------------------------------------
    @staticmethod
    def check_params(tensors, what, fp32=None):
        """every tensor on a ROCm device (``what`` names them); ``fp32``: the plan's name when its prepare reads raw fp32"""
        for t in tensors:
            _require_cuda(t, what)
            if fp32 and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise RuntimeError(f"{fp32}: parameters must be contiguous fp32")

    def check_compute_dtype(self):
        """``self.dtype`` (set by ``refresh()``) is still the module's compute dtype"""
        if dtype_code(self.module.compute_dtype) != self.dtype:
            raise RuntimeError(f"{self.who}: the model's compute dtype is now {self.module.compute_dtype!r} but the weights "
                               "were prepared in another one -- call refresh()")
