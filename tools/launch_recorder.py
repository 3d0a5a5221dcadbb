"""What the launch-trace tools share (decode_launch_trace.py, encoder_launch_trace.py): every public function of gritlm_amd.ops replaced
by a recorder that logs the call -- every argument of the op by name, defaults filled in; a tensor as (buffer by order of first
appearance, storage offset, shape, strides, dtype) -- and returns ``out`` or a stand-in, so the real host code runs to the end on CPU
tensors without a device."""
import inspect
import json
import types

import torch

from gritlm_amd import ops


class Recorder:
    """``with Recorder(returns) as r``: ops patched inside the block, ``r.out`` the launch list.  ``returns``: op name -> callable that
    takes the op's arguments and gives what the recorder hands back (default: the ``out`` argument).  ``values``: integer tensors of up
    to 64 elements are logged with their contents as well."""

    def __init__(self, returns=None, values=False):
        self.out, self.names, self.keep = [], {}, []
        self.returns, self.values = returns or {}, values

    def label(self, t):
        if isinstance(t, torch.Tensor):
            self.keep.append(t)                         # (alive to the end: a freed buffer's address would be handed out again)
            n = self.names.setdefault(t.untyped_storage().data_ptr(), len(self.names))
            lab = ["T", n, t.storage_offset(), list(t.shape), list(t.stride()), str(t.dtype)]
            if self.values and not t.dtype.is_floating_point and t.dtype != torch.bool and t.numel() <= 64:
                lab.append(t.reshape(-1).tolist())
            return lab
        if isinstance(t, (list, tuple)):
            return [self.label(x) for x in t]
        return t if t is None or isinstance(t, (bool, int, float, str)) else str(t)

    def log(self, name, args, kw):
        self.out.append([name, [self.label(x) for x in args], {k: self.label(v) for k, v in sorted(kw.items())}])

    def _rec(self, name):
        sig, ret = inspect.signature(self.saved[name]), self.returns.get(name)

        def f(*a, **k):
            full = sig.bind(*a, **k)                    # every argument of the op by name, defaults filled in: what the launch receives,
            full.apply_defaults()                       # however the call site spelled it
            self.log(name, [], full.arguments)
            return ret(*a, **k) if ret else full.arguments.get("out")
        return f

    def __enter__(self):
        self.saved = {n: v for n, v in vars(ops).items()
                      if isinstance(v, types.FunctionType) and not n.startswith("_") and v.__module__ == ops.__name__}
        for n in self.saved:
            setattr(ops, n, self._rec(n))
        return self

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            setattr(ops, n, v)


def canonical(tr) -> str:
    return json.dumps(tr, sort_keys=True, separators=(",", ":"))
