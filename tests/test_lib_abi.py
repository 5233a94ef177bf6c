"""CPU-side checks of the C-ABI library: builds for gfx950, loads, exports every declared symbol."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    syms = set()
    for fn in os.listdir(os.path.join(ROOT, "include")):
        txt = open(os.path.join(ROOT, "include", fn)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        syms |= set(re.findall(r"\b((?:tw|ppo|mg)_[a-z0-9_]+)\s*\(", txt))
    return syms


def _declarations():
    """(return type, name, [parameter declarations]) of every prototype in include/*.h, as the header spells them.  The
    headers are plain C with one declarator per parameter."""
    for fn in sorted(os.listdir(os.path.join(ROOT, "include"))):
        txt = open(os.path.join(ROOT, "include", fn)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
        for ret, name, params in re.findall(r"([A-Za-z_][\w \*\n]*?)\b((?:tw|ppo|mg)_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
            yield ret, name, [] if params.strip() == "void" else params.split(",")


def _prototypes():
    """{name: (return type, [parameter types])} of every prototype in include/*.h, each type as the header spells it
    with `const` and the parameter's name dropped and every pointer reduced to "*"."""
    def kind(decl, named):
        if "*" in decl:
            return "char *" if re.sub(r"\bconst\b", "", decl).split() == ["char", "*"] else "*"
        words = [w for w in decl.split() if w != "const"]
        return " ".join(words[:-1] if named else words)
    protos = {}
    for ret, name, params in _declarations():
        assert name not in protos, "%s is declared twice" % name
        protos[name] = (kind(ret, False), [kind(p, True) for p in params])
    return protos


def test_a_stream_parameter_is_spelled_stream_and_comes_last():
    """Every `void *` parameter whose name contains "stream" is named exactly `stream` and is its prototype's last one:
    tests/test_streams_gpu.py lists the entry points that take a stream by that spelling, and a prototype that spells it
    otherwise escapes its completeness test."""
    found, bad = 0, []
    for _, name, params in _declarations():
        for i, p in enumerate(params):
            m = re.fullmatch(r"\s*void\s*\*\s*(\w*stream\w*)\s*", p)
            if m:
                found += 1
                if m.group(1) != "stream" or i != len(params) - 1:
                    bad.append("%s: parameter %d of %d is `%s`" % (name, i + 1, len(params), p.strip()))
    assert not bad, "\n".join(bad)
    assert found >= 61, "only %d prototypes with a stream were found: the parser has lost them" % found


def test_ctypes_signatures_mirror_the_headers():
    """Every entry of _lib._SIGS against the prototype it mirrors: the parameter count, each parameter's class and the
    return type.  A pointer of any type is a ctypes pointer; an integer or floating type is the ctypes type of exactly
    that C type, so an `int` where the header says `int64_t` fails."""
    import ctypes as C
    import twoarmy_amd
    scalar = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
              "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double}

    def matches(ctype, kind, is_return):
        if kind == "char *" and is_return:
            return ctype is C.c_char_p
        if kind in ("*", "char *"):
            return ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer)
        return ctype is scalar[kind]                 # an unknown C type is a KeyError: extend the classes on purpose

    protos, sigs = _prototypes(), twoarmy_amd._lib._SIGS
    assert set(protos) == set(sigs) == _declared()
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        res, args = sigs[name]
        if not matches(res, ret, True):
            bad.append("%s returns %s, the table says %s" % (name, ret, res.__name__))
        if len(args) != len(params):
            bad.append("%s takes %d arguments, the table says %d" % (name, len(params), len(args)))
            continue
        bad += ["%s argument %d is %s, the table says %s" % (name, i, k, a.__name__)
                for i, (a, k) in enumerate(zip(args, params)) if not matches(a, k, False)]
    assert not bad, "\n".join(bad)


def test_library_loads_and_exports_all_declared_symbols():
    import __graft_entry__ as ge
    ge.build()
    import twoarmy_amd
    lib = twoarmy_amd._lib.lib()
    declared = _declared()
    assert "tw_step" in declared and "tw_rollout" in declared
    for s in sorted(declared):
        assert hasattr(lib, s), "libtwoarmy_hip.so lacks %s declared in include/" % s
    assert set(twoarmy_amd._lib.exported_symbols()) == declared
    assert lib.tw_version().startswith(b"twoarmy-hip")


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import twoarmy_amd
    from twoarmy_amd.engine import TwoarmyEngine
    with pytest.raises(twoarmy_amd._lib.TwoarmyLibraryError):
        TwoarmyEngine(6, 4)


def test_record_layout_matches_header():
    import twoarmy_amd
    txt = open(os.path.join(ROOT, "include", "twoarmy.h")).read()
    body = re.search(r"enum tw_field \{(.*?)\};", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    val, got = -1, {}
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            name, v = [s.strip() for s in item.split("=")]
            val = int(v)
        else:
            name, val = item, val + 1
        got[name[3:]] = val
    assert got == twoarmy_amd._lib.FIELDS


def test_ctypes_struct_mirrors_the_header():
    """struct tw_outputs as gcc lays it out from include/twoarmy.h == the ctypes mirror in _lib.py (size and offsets)."""
    import ctypes as C
    import subprocess
    import tempfile
    import twoarmy_amd
    fields = [f for f, _ in twoarmy_amd._lib.TwOutputs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "twoarmy.h"\nint main(void){printf("%zu", sizeof(tw_outputs));' + \
          "".join('printf(" %%zu", offsetof(tw_outputs, %s));' % f for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "a.c"), os.path.join(d, "a.out")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    T = twoarmy_amd._lib.TwOutputs
    assert vals[0] == C.sizeof(T)
    assert vals[1:] == [getattr(T, f).offset for f in fields]
