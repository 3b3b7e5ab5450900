"""`NativeModule`: the base of every module whose forward is a native engine — reference-layout
parameters plus the cache of the one `NativeEngine` built from them, dropped whenever the
parameters may have changed (load_state_dict, .to() / .float() / ..., a precision change)."""
import torch
import torch.nn as nn

from . import _lib
from .engine import NativeEngine


def _check_precision(precision):
    if precision not in _lib.DTYPES:
        raise ValueError(f"precision must be one of {sorted(_lib.DTYPES)}")


class NativeModule(nn.Module):
    """A subclass calls `_init_native(precision)` in its constructor and gets its engine from
    `_engine(device, key, make_desc, state_dict)`. One that caches more than engines extends
    `invalidate()`. (The counter is not called `_version`: that is torch's own class attribute,
    which state_dict() saves as the module's metadata.)"""

    def _init_native(self, precision):
        _check_precision(precision)
        self.precision = precision
        self._params_version = 0
        self._engines = {}
        self.register_load_state_dict_post_hook(lambda module, keys: module.invalidate())

    def invalidate(self):
        """The parameters may have changed: drop what was built from them."""
        self._params_version += 1
        self._engines = {}

    def _apply(self, fn, *args, **kwargs):
        r = super()._apply(fn, *args, **kwargs)
        self.invalidate()
        return r

    def set_precision(self, precision: str):
        _check_precision(precision)
        self.precision = precision
        self.invalidate()
        return self

    def _version_key(self):
        """The parameter versions of this module and of the NativeModules below it, in self.modules()
        order: a reload of a child alone (`model.backbone.load_state_dict(...)`) changes it too. Every
        forward asks for it, so it follows only children that are NativeModules themselves — where every
        class here keeps them — instead of walking the hundreds of plain parameter containers."""
        key = (self._params_version,)
        for m in self._modules.values():
            if isinstance(m, NativeModule):
                key += m._version_key()
        return key

    def _engine(self, device, key, make_desc, state_dict):
        """The engine of (`device`, `key`, precision, parameter versions): the cached one, or a new one
        built from make_desc() and state_dict(), which replaces it (one engine is kept)."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        key = (index, *key, self.precision, self._version_key())
        eng = self._engines.get(key)
        if eng is None:
            eng = NativeEngine(make_desc(), state_dict(), index)
            self._engines = {key: eng}
        return eng
