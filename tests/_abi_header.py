"""What the ABI tests of the side units share (tests/test_*_abi_cpu.py): the names a C header declares and the text of its
macros, and the checks every unit's boundary passes.  A plain helper module: it holds no test."""
import ast
import ctypes as ct
import inspect
import pickle
import re

import pytest

from sbayes_amd import _handle, _lib


def declared(header_text):
    """The sbe_* functions the header declares, sorted (comments are not looked at)."""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return sorted(set(re.findall(r"\b(sbe_[a-z0-9_]+)\s*\(", text)))


def macro(header_text, name):
    """The replacement text of `#define name`, without its trailing comment."""
    return re.search(rf"#define {name}\s+(.+?)\s*(?:/\*|$)", header_text, flags=re.M).group(1)


def check_symbols(module, header_text, count):
    """The `count` sbe_* functions the unit's header declares are exported by the library and bound by the module's own
    prototype table, which leaves the engine's alone, and the library, the module and the header state one ABI version.
    Returns the names."""
    lib = module.load()
    names = declared(header_text)
    assert len(names) == count, names
    for name in names:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert sorted(module.PROTOTYPES) == names
    version = next(name for name in names if name.endswith("_abi_version"))
    assert getattr(lib, version)() == module.ABI_VERSION == int(macro(header_text, version.upper()))
    assert not set(names) & set(_lib.PROTOTYPES)          # the engine's table is not extended
    return names


def check_ptr_arguments(module):
    """The module and sbayes_amd/_handle.py pass bare addresses (_ptr): every argument must be a plain local name, never a
    temporary."""
    for source in (module, _handle):
        tree = ast.parse(inspect.getsource(source))
        calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "_ptr"]
        bad = [(n.lineno, ast.unparse(n)) for n in calls if len(n.args) != 1 or not isinstance(n.args[0], ast.Name)]
        assert calls and not bad, (source.__name__, bad)


def check_not_picklable(handle_class):
    h = object.__new__(handle_class)
    h._h = ct.c_void_p()
    with pytest.raises(TypeError, match="not picklable"):
        pickle.dumps(h)


NUMBERS = (ct.c_int, ct.c_int64, ct.c_uint64, ct.c_float, ct.c_double)     # every other argument type of the tables is a pointer


def check_null_handles(module, text=b"null handle"):
    """Every entry point of the module's table that takes the unit's handle and returns a code refuses a null handle with
    SBE_ERR_ARG and `text`, whatever the other arguments are (zeros and nulls here); a create that takes only a device
    refuses a null `out` and a negative device.  Returns the names of the entry points called."""
    lib = module.load()
    last_error = getattr(lib, next(name for name in module.PROTOTYPES if name.endswith("_last_error")))
    called = []
    for name, (restype, argtypes) in module.PROTOTYPES.items():
        if name.endswith("_create") and argtypes == [ct.POINTER(_handle.c_handle_p), ct.c_int]:
            h = ct.c_void_p()
            assert getattr(lib, name)(None, 0) == 1
            assert b"null pointer argument: out" in last_error(None)
            assert getattr(lib, name)(ct.byref(h), -1) == 1 and not h
            assert b"device -1 out of range" in last_error(None)
            called.append(name)
        elif restype is ct.c_int and argtypes and argtypes[0] is _handle.c_handle_p:
            rest = [0 if t in NUMBERS else None for t in argtypes[1:]]
            assert getattr(lib, name)(None, *rest) == 1, name
            assert text in last_error(None), name
            called.append(name)
    return called
