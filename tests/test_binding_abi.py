"""mlhot/binding.py held to include/mlhot.h, without a GPU: the signature table against the header's prototypes, the struct
mirrors against the compiler's sizeof / offsetof, what a loaded library ends up with, and what a library that lacks the entries
added within the ABI version does.  A wrong argtypes entry or a shifted field is a GPU fault at run time; here it is a failed
assertion."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

from mlhot import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# C name -> mirror, for every struct of the header that the binding fills field by field
STRUCTS = {"mlhot_enc_params": B.EncParams, "mlhot_enc_grads": B.EncGrads, "mlhot_chain_layer": B.ChainLayer,
           "mlhot_chain_grads": B.ChainGrads, "mlhot_linear_job": B.LinearJob, "mlhot_rows_src": B.RowsSrc,
           "mlhot_trunk_wset": B.TrunkWset, "mlhot_trunk_pass": B.TrunkPass, "mlhot_bbb_item": B.BbbItem, "mlhot_np_dims": B.NpDims,
           "mlhot_np_params": B.NpParams, "mlhot_np_grads": B.NpGrads, "mlhot_loss_desc": B.LossDesc}
# the records mlhot/augment.py builds as int32 / uint8 tensors: the binding knows their size only
BYTES = {"mlhot_aug_record": B.AUG_RECORD_BYTES, "mlhot_aug_record_img": B.AUG_IMG_RECORD_BYTES, "mlhot_colour_tabs": B.COLOUR_TABS_BYTES}
CONSTANTS = {"MLHOT_ABI_VERSION": B.ABI_VERSION, "MLHOT_HEADS": B.HEADS, "MLHOT_MAX_HIDDEN": B.MAX_HIDDEN}
SCALARS = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "long": C.c_long, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}


def _header():
    """include/mlhot.h without comments and preprocessor lines."""
    with open(os.path.join(INCLUDE, "mlhot.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return "\n".join(line for line in re.sub(r"//[^\n]*", " ", text).split("\n") if not line.lstrip().startswith("#"))


def _kind(decl):
    """'pointer' or the ctypes class of one C parameter / return type (the parameter's name, if any, is dropped)."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert words and words[0] in SCALARS, f"the ABI test does not know the C type in {decl!r}"
    return SCALARS[words[0]]


def header_prototypes():
    """name -> (kind of the return type, [kind of every parameter]) for each `ret name(args);` of the header."""
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?\w+[\s*]+)(mlhot_\w+)\s*\(([^()]*)\)\s*;", _header()):
        assert name not in protos, f"{name} is declared twice"
        args = [a.strip() for a in args.split(",")]
        protos[name] = (_kind(ret), [] if args == ["void"] else [_kind(a) for a in args])
    return protos


def _agrees(ctype, kind):
    if kind == "pointer":
        return ctype in (C.c_void_p, C.c_char_p) or (inspect.isclass(ctype) and issubclass(ctype, C._Pointer))
    return ctype is kind


def test_signature_table_agrees_with_the_header():
    protos = header_prototypes()
    assert len(protos) >= 82                                   # a parser that silently matches nothing must not pass
    assert len(set(re.findall(r"\b(mlhot_[a-z0-9_]+)\s*\(", _header()))) == len(protos)        # ... nor one that misses a prototype
    assert sorted(B.SIGNATURES) == sorted(protos), set(B.SIGNATURES) ^ set(protos)
    assert list(B.SIGNATURES) == list(protos), "the table is kept in the header's order"
    for name, (ret, params) in protos.items():
        restype, argtypes = B.SIGNATURES[name]
        assert _agrees(restype, ret), f"{name}: restype {restype} against the header's {ret}"
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        for k, (have, want) in enumerate(zip(argtypes, params)):
            assert _agrees(have, want), f"{name}: argument {k} is {have}, the header has {want}"


def _compile(tmp_path, name, source, *flags):
    src, out = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text(source)
    subprocess.run(["g++", "-std=c++17", "-I", INCLUDE, *flags, str(src), "-o", str(out)], check=True)
    return str(out)


def test_struct_mirrors_and_constants_agree_with_the_compiler(tmp_path):
    """sizeof of every struct, offsetof and size of every field, and the header's constants, as the host compiler sees the header.
    A renamed field does not compile; a reordered, retyped or missing one shows as a mismatch."""
    mirrors = {cls for _, cls in inspect.getmembers(B, inspect.isclass) if issubclass(cls, C.Structure) and cls is not C.Structure}
    assert mirrors == set(STRUCTS.values()), "a struct mirror of mlhot/binding.py is not in this test's STRUCTS"
    in_header = set(re.findall(r"\}\s*(mlhot_\w+)\s*;", _header()))
    assert in_header == set(STRUCTS) | set(BYTES), in_header ^ (set(STRUCTS) | set(BYTES))
    want, lines = {}, []
    for cname, size in list(BYTES.items()) + [(n, C.sizeof(cls)) for n, cls in STRUCTS.items()]:
        want[f"sizeof {cname}"] = size
        lines.append(f'printf("sizeof {cname} %zu\\n", sizeof({cname}));')
    for cname, cls in STRUCTS.items():
        for field in (f[0] for f in cls._fields_):
            want[f"offsetof {cname}.{field}"] = getattr(cls, field).offset
            want[f"sizeof {cname}.{field}"] = getattr(cls, field).size
            lines.append(f'printf("offsetof {cname}.{field} %zu\\n", offsetof({cname}, {field}));')
            lines.append(f'printf("sizeof {cname}.{field} %zu\\n", sizeof((({cname}*)0)->{field}));')
    for macro, value in CONSTANTS.items():
        want[f"value {macro}"] = value
        lines.append(f'printf("value {macro} %zu\\n", (size_t)({macro}));')
    exe = _compile(tmp_path, "layout", '#include <stdio.h>\n#include "mlhot.h"\nint main() {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    got = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        what, _, value = line.rpartition(" ")
        got[what] = int(value)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"(compiler, binding): {wrong}"


def test_loaded_library_carries_every_signature(hostsim):
    assert hostsim.missing == set()
    for name, (restype, argtypes) in B.SIGNATURES.items():
        fn = getattr(hostsim.c, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype, name


def test_library_without_the_later_entries_loads_and_says_what_it_lacks(tmp_path, monkeypatch):
    """A prebuilt library of the right ABI version that predates the entries added within it: MlhotLib loads it, and the wrappers
    of those entries raise MlhotError naming the symbol - no AttributeError, no call through an undeclared pointer."""
    stub = _compile(tmp_path, "libstub.so", '''#include "mlhot.h"
int mlhot_version(void) { return MLHOT_ABI_VERSION; }
const char* mlhot_last_error(void) { return ""; }
size_t mlhot_np_struct_bytes(int which) {
  const size_t bytes[6] = {sizeof(mlhot_np_dims), sizeof(mlhot_np_params), sizeof(mlhot_np_grads), sizeof(mlhot_chain_layer),
                           sizeof(mlhot_chain_grads), sizeof(mlhot_linear_job)};
  return which >= 0 && which < 6 ? bytes[which] : 0;
}
''', "-shared", "-fPIC")
    monkeypatch.setattr(B.MlhotLib, "_last", B.MlhotLib._last)       # the static test helpers keep the library they had
    lib = B.MlhotLib(stub)
    assert lib.missing == set(B.SIGNATURES) - {"mlhot_version", "mlhot_last_error", "mlhot_np_struct_bytes"}
    u8 = torch.zeros(1, 4, 4, 1, dtype=torch.uint8)
    for call in (lambda: lib.agg_prefix_fwd("mean", torch.zeros(1, 2, 4)),
                 lambda: lib.linear_rows_supported(4, 0, 4),
                 lambda: lib.favor_prefix_ws_bytes(1, 1, 1, 1, 16, 16),
                 lambda: lib.augment_ingest_u8(u8, torch.zeros(1, 32, dtype=torch.int32)),
                 lambda: lib.augment_ingest_u8_img(u8, torch.zeros(1, 40, dtype=torch.int32))):
        with pytest.raises(B.MlhotError, match="lacks mlhot_"):
            call()


def test_signatures_are_declared_in_one_place():
    """The loop in MlhotLib.__init__ is the only code of the binding that assigns a signature."""
    source = inspect.getsource(B)
    assert len(re.findall(r"\.(?:argtypes|restype)\s*=(?!=)", source)) <= 2
    assert len(re.findall(r"\.(?:argtypes|restype)\s*=(?!=)", inspect.getsource(B.MlhotLib.__init__))) == 2
