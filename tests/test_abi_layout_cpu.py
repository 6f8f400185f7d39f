"""The ctypes mirror in recon_amd/_lib.py against include/recon_hip.h: size and field offsets of every struct as a C compiler lays the
header's out, and parameter count and return type of every prototype.  A field or an argument present on one side only would otherwise
be silent memory corruption on the device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

# ctypes class in recon_amd/_lib.py -> struct typedef in include/recon_hip.h
STRUCTS = {
    "ReconGraph": "recon_graph",
    "GatFwdArgs": "recon_gat_fwd_args",
    "GatBwdArgs": "recon_gat_bwd_args",
    "GatAtpArgs": "recon_gat_atp_args",
    "GatAtpBwdArgs": "recon_gat_atp_bwd_args",
    "PropArgs": "recon_prop_args",
    "PropBwdArgs": "recon_prop_bwd_args",
    "PropB16Args": "recon_prop_b16_args",
    "PropB16BwdArgs": "recon_prop_b16_bwd_args",
    "ReconKG": "recon_kg",
    "GcnArgs": "recon_gcn_args",
    "GcnBwdArgs": "recon_gcn_bwd_args",
    "GcnB16Args": "recon_gcn_b16_args",
    "GcnB16BwdArgs": "recon_gcn_b16_bwd_args",
    "GcnB16StackArgs": "recon_gcn_b16_stack_args",
    "GcnB16StackTrainArgs": "recon_gcn_b16_stack_train_args",
}
RESTYPES = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "const char*": ctypes.c_char_p}


def _header():
    text = open(os.path.join(ROOT, "include", "recon_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_every_structure_and_every_header_struct_is_mapped():
    from recon_amd import _lib
    classes = {n for n, c in vars(_lib).items() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}
    assert classes == set(STRUCTS), classes ^ set(STRUCTS)
    typedefs = set(re.findall(r"\}\s*(recon_[a-z0-9_]+)\s*;", _header()))
    assert typedefs == set(STRUCTS.values()), typedefs ^ set(STRUCTS.values())


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_struct_sizes_and_field_offsets_match_the_header(tmp_path):
    from recon_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "recon_hip.h"', 'int main(void) {']
    for cls, struct in STRUCTS.items():
        lines.append('  printf("%s sizeof %%lu\\n", (unsigned long)sizeof(%s));' % (cls, struct))
        for field, _ in getattr(_lib, cls)._fields_:
            lines.append('  printf("%s %s %%lu\\n", (unsigned long)offsetof(%s, %s));' % (cls, field, struct, field))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    in_c = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        cls, field, value = line.split()
        in_c[cls, field] = int(value)
    for cls in STRUCTS:
        c = getattr(_lib, cls)
        assert ctypes.sizeof(c) == in_c[cls, "sizeof"], "%s (%s): sizeof %d in ctypes, %d in C" % (cls, STRUCTS[cls], ctypes.sizeof(c), in_c[cls, "sizeof"])
        for field, _ in c._fields_:
            off = getattr(c, field).offset
            assert off == in_c[cls, field], "%s.%s (%s): offset %d in ctypes, %d in C" % (cls, field, STRUCTS[cls], off, in_c[cls, field])
    assert len(in_c) == sum(1 + len(getattr(_lib, cls)._fields_) for cls in STRUCTS)


def test_prototypes_match_the_bound_signatures():
    from recon_amd import _lib
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\s*\b(recon_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()):
        params = params.strip()
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), 0 if params in ("", "void") else params.count(",") + 1)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert set(protos) == set(bound), set(protos) ^ set(bound)
    for name, (ret, n_params) in sorted(protos.items()):
        res, args = bound[name]
        assert n_params == len(args), "%s: %d parameters in the header, %d argtypes" % (name, n_params, len(args))
        assert ret in RESTYPES, "%s: return type %r has no ctypes counterpart here" % (name, ret)
        assert res is RESTYPES[ret], "%s: returns %s in the header, restype %s" % (name, ret, res.__name__)
