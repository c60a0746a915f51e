"""What the owners of a device handle share: Engine (prefix `sbe`) and the handle classes of the side units (prefix
`sbe_<unit>`).  Every handle type of the C ABI has <prefix>_create, <prefix>_destroy and
<prefix>_last_error with the same conventions (include/sbe_engine.h, "Errors"), and every owner follows the package's
process model (sbayes_amd/_proc.py): created in the process that uses it, registered there, never pickled, forgotten --
not destroyed -- in a fork()ed child."""
from __future__ import annotations

import ctypes as ct
import os

from . import _fast, _lib, _proc

c_handle_p = ct.c_void_p                 # every handle type of the C ABI is opaque
_ptr = _fast.addr                        # buffer address as a plain int (every array argument is c_void_p)


class EngineError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"sbe error {code}: {message}")
        self.code = code


_BOUND = {}                              # unit prefix -> the library object its prototypes were last attached to


def bind(prefix, prototypes, abi_version):
    """The engine library with the prototype table (name -> (restype, argtypes)) of the unit whose entry points start with
    `prefix` attached, and the unit's ABI version checked; both once per loaded library."""
    lib = _lib.load()
    if _BOUND.get(prefix) is not lib:
        for name, (restype, argtypes) in prototypes.items():
            fn = getattr(lib, name)       # AttributeError if the library lacks a declared symbol
            fn.restype = restype
            fn.argtypes = argtypes
        found = getattr(lib, prefix + "_abi_version")()
        if found != abi_version:
            raise RuntimeError(f"sbayes_amd.{prefix[4:]}: ABI version mismatch ({found} != {abi_version})")
        _BOUND[prefix] = lib
    return lib


def unit_prototypes(prefix):
    """The rows every side unit's prototype table has (name -> (restype, argtypes)); the unit adds <prefix>_create and its own."""
    return {
        f"{prefix}_abi_version": (ct.c_int, []),
        f"{prefix}_last_error": (ct.c_char_p, [c_handle_p]),
        f"{prefix}_destroy": (ct.c_int, [c_handle_p]),
        f"{prefix}_last_kernel_ms": (ct.c_int, [c_handle_p, ct.POINTER(ct.c_float)]),
    }


def store_prototypes(prefix, shape):
    """unit_prototypes and the rows every unit with a row store adds: create on a device, reset (`shape`: its argument types
    behind the lane count), append_rows and rows of a lane."""
    return {
        **unit_prototypes(prefix),
        f"{prefix}_create": (ct.c_int, [ct.POINTER(c_handle_p), ct.c_int]),
        f"{prefix}_reset": (ct.c_int, [c_handle_p, ct.c_int, *shape]),
        f"{prefix}_append_rows": (ct.c_int, [c_handle_p, ct.c_int, ct.c_void_p, ct.c_int64]),
        f"{prefix}_rows": (ct.c_int, [c_handle_p, ct.c_int, ct.POINTER(ct.c_int64)]),
    }


class DeviceHandle:
    """Owner of one handle of the C ABI.  A subclass names the handle type and calls _create from its __init__, after it has
    validated its arguments; close(), __del__ and _forget work on an object whose __init__ never got that far."""

    _prefix = "sbe"                       # the handle type's entry points are <_prefix>_create, _destroy, _last_error
    _noun = "a device handle"             # subject of the message that refuses pickling

    def _fn(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def _create(self, load, *args):
        """<prefix>_create(&handle, *args) on the library that `load` returns."""
        _proc.check_usable()             # ForkedWithHipError in a fork()ed child of a HIP-initialised parent
        self._lib = load()
        self._h = ct.c_void_p()
        self._pid = None                 # pid of the process the handle lives in (set once the create succeeded)
        # marked on the ATTEMPT, not on success: a create that fails after the runtime came up (out of memory, a bad shape
        # behind hipSetDevice) has initialised HIP all the same, and a child forked afterwards must not be taken for a
        # fresh process
        _proc.mark_hip_touched()
        rc = self._fn("create")(ct.byref(self._h), *args)
        if rc != 0:
            msg = self._fn("last_error")(None)
            self._h = ct.c_void_p()
            raise EngineError(rc, msg.decode() if msg else f"{self._prefix}_create failed")
        self._pid = os.getpid()
        _proc.register_engine(self)

    def _last_error(self):
        msg = self._fn("last_error")(self._h)
        return msg.decode() if msg else "?"

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self._last_error())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if self._pid == os.getpid():         # (a handle that reached another process by any road is never destroyed there)
                self._fn("destroy")(self._h)
            self._h = ct.c_void_p()

    def _forget(self, lib_face):
        """After fork(), in the child (_proc._after_fork_in_child): drop the inherited handle WITHOUT destroying it -- its
        device memory and stream belong to the parent -- and make every later call on this object raise."""
        self._h = ct.c_void_p()
        self._lib = lib_face

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __getstate__(self):
        raise TypeError(f"{self._noun} holds device memory and is not picklable; re-create it in the new process")


class UnitHandle(DeviceHandle):
    """Owner of a side unit's handle: those live on one device (self.device) and also have <prefix>_last_kernel_ms."""

    def _create_on(self, load, device, *args):
        """<prefix>_create(&handle, device, *args); device None: the device of the process's engine (registry.default_device)."""
        if device is None:
            from .registry import default_device
            device = default_device()
        self.device = int(device)
        self._create(load, self.device, *args)

    def last_kernel_ms(self) -> float:
        """Device time of the unit's kernels in the last compute call (HIP events)."""
        ms = ct.c_float(0)
        self._check(self._fn("last_kernel_ms")(self._h, ct.byref(ms)))
        return float(ms.value)


class RowStoreHandle(UnitHandle):
    """Owner of a unit handle that stores rows per lane (the chains of a column store, the runs of a sample store).  A
    subclass names a lane in the messages (_lane), counts its lanes (_lane_count()) and has reset(*shape) and
    append(lane, rows)."""

    _lane = "lane"

    def rows(self, lane) -> int:
        n = ct.c_int64(0)
        self._check(self._fn("rows")(self._h, int(lane), ct.byref(n)))
        return n.value

    def _check_lane(self, lane):
        lane, count = int(lane), self._lane_count()
        if not 0 <= lane < count:
            raise ValueError(f"{self._lane} {lane} out of range [0, {count})")
        return lane

    def _append_rows(self, lane, block):
        """<prefix>_append_rows of a checked block (rows along its first axis); returns the library's code."""
        return self._fn("append_rows")(self._h, lane, _ptr(block), block.shape[0])

    @classmethod
    def filled(cls, device, shape, blocks):
        """A new handle on `device`, reset to `shape`, with blocks[lane] appended to every lane.  The caller closes it; it is
        closed here if any of that raises."""
        h = cls(device)
        try:
            h.reset(*shape)
            for lane, block in enumerate(blocks):
                h.append(lane, block)
        except BaseException:
            h.close()
            raise
        return h


# ---- one handle per device, created lazily (assoc.py, geo.py): device -> handle; per process, emptied in a fork()ed child --
def device_cache():
    cache = {}
    _proc.on_fork_clear(cache.clear)
    return cache


def cached_handle(cache, make, device):
    """The handle on `device` in `cache`, made by make(device) on first use (or after it was closed)."""
    h = cache.get(int(device))
    if h is None or not h._h:
        h = cache[int(device)] = make(device)
    return h


def release_cached(cache):
    for h in list(cache.values()):
        h.close()
    cache.clear()
