"""salva_amd._lib.host_out / device_out: the ...Out structs of the device queries over host arrays and over device addresses.  The
element type of every pointer field is read from the struct; only ctypes and numpy are needed, no library and no device."""
import ctypes as C
import inspect

import numpy as np
import pytest

from salva_amd import _lib

UINT32_FIELDS = {"count", "fluid", "index", "kind", "id", "triangles"}
OUT_STRUCTS = [cls for name, cls in inspect.getmembers(_lib, inspect.isclass) if name.endswith("Out") and issubclass(cls, C.Structure)]
POINTER_FIELDS = [(cls, name) for cls in OUT_STRUCTS for name, t in cls._fields_ if isinstance(t, type) and issubclass(t, C._Pointer)]


def address(pointer):
    return C.cast(pointer, C.c_void_p).value


def test_every_out_struct_is_covered():
    assert {cls.__name__ for cls in OUT_STRUCTS} == {"RayOut", "FieldOut", "SurfaceOut", "AnisotropyOut", "AnisoFieldOut", "DiffusePotentialsOut",
                                                     "DiffuseOut"}
    assert UINT32_FIELDS <= {name for _, name in POINTER_FIELDS}


@pytest.mark.parametrize("cls,name", POINTER_FIELDS, ids=[f"{cls.__name__}.{name}" for cls, name in POINTER_FIELDS])
def test_host_out_of_one_field(cls, name):
    arrays, out, room = _lib.host_out(cls, {name: (5, 3)})
    assert set(arrays) == {name} and not room
    a = arrays[name]
    assert a.dtype == (np.uint32 if name in UINT32_FIELDS else np.float32) and a.shape == (5, 3) and not a.any()
    assert address(getattr(out, name)) == a.ctypes.data
    for other_cls, other in POINTER_FIELDS:
        if other_cls is cls and other != name:
            assert not getattr(out, other)  # (a field not asked for is null)
    # an empty shape: a pointer the library can name, kept in `room`, and an empty array for the caller
    arrays, out, room = _lib.host_out(cls, {name: (0, 3)})
    assert arrays[name].shape == (0, 3) and arrays[name].dtype == a.dtype
    assert len(room) == 1 and room[0].size and room[0].dtype == a.dtype and address(getattr(out, name)) == room[0].ctypes.data


@pytest.mark.parametrize("cls", OUT_STRUCTS, ids=lambda cls: cls.__name__)
def test_device_out_sets_the_addresses_given(cls):
    names = [name for c, name in POINTER_FIELDS if c is cls]
    given = {name: (0x1000 * (k + 1) if k % 2 == 0 else 0) for k, name in enumerate(names)}
    out = _lib.device_out(cls, dict(given, no_such_field=0x7000))
    for name in names:
        assert (address(getattr(out, name)) or 0) == given[name], name
    assert not hasattr(out, "no_such_field")
    assert all(getattr(out, name) == 0 for name, t in cls._fields_ if name not in names)  # (capacities untouched)
