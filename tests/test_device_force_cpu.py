"""User-defined forces on the device (SALVA_HIP_FORCE_DEVICE, include/salva_hip.h), the part that needs no GPU: the
view's layout is the same in the C header, the library (a static_assert against the header's constant) and the ctypes mirror; the
plugin of examples/device_forces3.hip is built with everything else and exports its two entry points; the header for user kernels
compiles on its own for gfx950."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PLUGIN = os.path.join(ROOT, "examples", "libdevice_forces3.so")


def _header_constant(name):
    src = open(os.path.join(ROOT, "include", "salva_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


def test_view_layout_is_the_headers(tmp_path):
    from salva_amd import _lib

    assert C.sizeof(_lib.DeviceView) == _header_constant("SALVA_HIP_DEVICE_VIEW_BYTES") == _lib.DEVICE_VIEW_BYTES
    assert _header_constant("SALVA_HIP_DEVICE_VIEW_VERSION") == _lib.DEVICE_VIEW_VERSION
    assert _lib.FORCE_DEVICE == 9
    # the C compiler's own answer, field by field: size and the offset of every member the mirror names
    fields = [f[0] for f in _lib.DeviceView._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n  printf("%%zu", sizeof(SalvaHipDeviceView));\n%s  return 0;\n}\n'
            % (os.path.join(ROOT, "include", "salva_hip.h"),
               "".join('  printf(" %%zu", offsetof(SalvaHipDeviceView, %s));\n' % f for f in fields)))
    src, exe = tmp_path / "view.c", tmp_path / "view"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_lib.DeviceView)
    assert got[1:] == [getattr(_lib.DeviceView, f).offset for f in fields]
    # and the library asserts the same constant where it fills the struct
    capi = open(os.path.join(ROOT, "salva_amd", "csrc", "capi.hip")).read()
    assert re.search(r"static_assert\(sizeof\(SalvaHipDeviceView\)\s*==\s*SALVA_HIP_DEVICE_VIEW_BYTES", capi)


def test_plugin_is_built_and_exports_its_entry_points(hip_lib):
    assert os.path.exists(PLUGIN), "examples/Makefile builds it (build())"
    lib = C.CDLL(PLUGIN)
    for name in ("df3_field", "df3_xsph"):
        assert hasattr(lib, name), name


def test_new_entry_points_are_exported_and_the_mirror_knows_them(hip_lib):
    from salva_amd import DeviceForce, PluginForce, _lib

    for name in ("salva_hip_set_device_force_callback", "salva_hip_device_view_read", "salva_hip_get_device_force_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    d = PluginForce(PLUGIN, "df3_field", 0, [0.3, 0.4, -0.2])._desc()
    assert d.kind == _lib.FORCE_DEVICE and d.p[0] == 0.0 and abs(d.p[2] - 0.4) < 1e-7
    assert DeviceForce(7)._desc().p[0] == 7.0
    with pytest.raises(ValueError):
        DeviceForce(8)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_device_header_compiles_on_its_own():
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-command-line-argument", "-fsyntax-only", "-x", "hip",
                           os.path.join(ROOT, "include", "salva_hip_device.h")])
