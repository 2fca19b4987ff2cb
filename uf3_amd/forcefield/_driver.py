"""
What the classes around a library-owned state share (``MolecularDynamics``, ``Relaxation``, ``NudgedElasticBand``,
``MonteCarlo``): the argument checks, which raise ``ValueError("<who>: ...")`` with ``who`` the class the user called, and
``Driver``, the life cycle of a handle of ``libuf3hip.so``.
"""
import ctypes as C
import numbers
import os

import numpy as np

from uf3_amd import _lib


def frames_of(who, atoms_or_list):
    frames = list(atoms_or_list) if isinstance(atoms_or_list, (list, tuple)) else [atoms_or_list]
    if not frames:
        raise ValueError(f"{who}: no frames")
    for k, a in enumerate(frames):
        if len(a) < 1:
            raise ValueError(f"{who}: frame {k} has no atoms")
    return frames


def check_real(who, name, value, lo=0.0, strict=False, hi=None):
    """``value`` as a finite float, > ``lo`` (``strict``) or >= ``lo`` (``lo`` None: unbounded below) and <= ``hi``."""
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a number") from None
    if not np.isfinite(x) or (lo is not None and (x <= lo if strict else x < lo)) or (hi is not None and x > hi):
        bound = "" if lo is None else (f" and > {lo}" if strict else f" and >= {lo}")
        raise ValueError(f"{who}: {name} must be finite{bound}" + (f" and <= {hi}" if hi is not None else "") + f", got {value!r}")
    return x


def check_int(who, name, value, lo=0, hi=None):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{who}: {name} must be an integer >= {lo}" + (f" and <= {hi}" if hi is not None else "") + f", got {value!r}")
    return int(value)


def check_mask(who, name, mask, n_atoms):
    """A boolean mask over the concatenated atoms as the library takes it (uint8 [n_atoms]); None stays None."""
    if mask is None:
        return None
    m = np.asarray(mask)
    if m.dtype != bool:
        raise ValueError(f"{who}: {name} must be a boolean mask over the concatenated atoms")
    m = m.reshape(-1)
    if m.size != n_atoms:
        raise ValueError(f"{who}: {name} holds {m.size} entries for {n_atoms} atoms")
    return np.ascontiguousarray(m.astype(np.uint8))


class Driver:
    """A handle created by ``uf3_<KIND>_create`` on ``self._batch``, read by ``uf3_<KIND>_get_state`` and freed by
    ``uf3_<KIND>_destroy``.  A subclass checks every argument and builds ``self._batch`` before it calls ``_create``, the first
    touch of the device."""
    KIND = None
    handle = None                   # (there before anything in a subclass's __init__ can raise: close() is always safe)

    def _create(self, calculator, device, head, tail=()):
        """``head``, ``tail``: what the library's create function takes between the frames and the model's coefficients, and
        between those and the handle it returns."""
        self.ctx = _lib.get_context(calculator.device if device is None else device)
        self._dbasis = _lib.device_basis(calculator.bspline_config, self.ctx)
        self._pid = os.getpid()
        h = C.c_void_p()
        create = getattr(self.ctx.lib, f"uf3_{self.KIND}_create")
        model = [_lib._p(c) for c in (calculator._c1, calculator._c2, calculator._c3)]
        self.ctx.check(create(self._dbasis.handle, C.byref(self._batch.struct), *head, *model, *tail, C.byref(h)))
        self.handle = h

    def _live(self):
        if not self.handle:
            raise RuntimeError(f"{self.WHO}: the object is closed")
        return self.handle

    def close(self):
        if self.handle:
            # (a forked child, or a context already gone: the handle is not this process's to free)
            if os.getpid() == self._pid and self.ctx.handle:
                getattr(self.ctx.lib, f"uf3_{self.KIND}_destroy")(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fetch(self, shapes, which):
        """The entries ``which`` of ``shapes`` ({name: (shape, dtype)} in the order of ``uf3_<KIND>_get_state``'s arguments)."""
        out = {k: np.empty(*shapes[k]) for k in which}
        get_state = getattr(self.ctx.lib, f"uf3_{self.KIND}_get_state")
        self.ctx.check(get_state(self._live(), *[_lib._p(out[k]) if k in out else None for k in shapes]))
        return out
