"""CPU: the C-ABI library builds, loads and exports every symbol include/decomp_hip.h
declares, and the ctypes table binds every one of them with the header's types (no compute
call is made here: there is no GPU in the CPU test tier)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(dcp_[a-z0-9_]+)\s*\(', text)))


def test_header_symbols_exported_and_bound():
    from decomp_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), 'header declares %s but the library does not export it' % n
        assert n in _hip.SIGNATURES, 'no ctypes signature for %s' % n
    for n in _hip.SIGNATURES:
        assert n in names, '%s is bound but not declared in the header' % n


# C type -> ctypes type.  A pointer may also be bound as c_void_p (device arrays and the handle are).
_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double, 'float': ctypes.c_float,
            'unsigned': ctypes.c_uint}
_POINTEES = dict(_SCALARS, int32_t=ctypes.c_int32, uint32_t=ctypes.c_uint32, void=None, dcp_handle=None)
_RETURNS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p}


def _prototypes(text):
    """[(return type, name, [argument, ...])] of every function the header text declares.  Whatever is left after
    the comments, the preprocessor lines, the enums and the extern "C" braces must be a typedef or a prototype."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    text = re.sub(r'\benum\s*\{[^}]*\}\s*;', '', text)
    text, n_open = re.subn(r'extern\s+"C"\s*\{', '', text)
    assert n_open == 1 and text.count('}') == 1 and text.rstrip().endswith('}'), 'unexpected braces in the header'
    out = []
    for stmt in text.rstrip()[:-1].split(';'):
        stmt = ' '.join(stmt.split())
        if not stmt or stmt.startswith('typedef '):
            continue
        m = re.fullmatch(r'(.*?)\b(dcp_[a-z0-9_]+) ?\(([^()]*)\)', stmt)
        assert m, 'cannot parse this declaration of the header: %r' % stmt
        args = m.group(3).strip()
        out.append((m.group(1).replace(' *', '*').strip(), m.group(2),
                    [] if args in ('', 'void') else [a.strip() for a in args.split(',')]))
    return out


def _arg_matches(arg, ctype):
    """Does the C parameter `arg` (type and name) agree with the bound ctypes type?  Raises on a C type without a
    rule, so that a new kind of argument cannot pass unchecked."""
    arg = ' '.join(re.sub(r'\bconst\b', ' ', arg).replace('*', ' * ').split())
    tokens = arg.split(' ')
    assert len(tokens) >= 2 and re.fullmatch(r'[A-Za-z_]\w*', tokens[-1]), 'cannot parse the parameter %r' % arg
    base, stars = tokens[0], tokens[1:-1]
    assert all(s == '*' for s in stars), 'cannot parse the parameter %r' % arg
    if not stars:
        if base == 'dcp_allreduce_fn':
            return ctype is ctypes.c_void_p
        assert base in _SCALARS, 'no rule for the C type %r' % base
        return ctype is _SCALARS[base]
    assert base in _POINTEES, 'no rule for a pointer to the C type %r' % base
    if len(stars) == 2:
        assert base == 'dcp_handle', 'no rule for %r' % arg
        return ctype is ctypes.POINTER(ctypes.c_void_p)
    pointee = _POINTEES[base]
    return ctype is ctypes.c_void_p or (pointee is not None and ctype is ctypes.POINTER(pointee))


def _mismatches(prototypes, signatures):
    bad = []
    for ret, name, args in prototypes:
        assert ret in _RETURNS, 'no rule for the return type %r of %s' % (ret, name)
        if name not in signatures:
            bad.append('%s: not bound' % name)
            continue
        restype, argtypes = signatures[name]
        if restype is not _RETURNS[ret]:
            bad.append('%s: returns %s, bound as %s' % (name, ret, restype))
        if len(args) != len(argtypes):
            bad.append('%s: %d arguments, %d bound' % (name, len(args), len(argtypes)))
            continue
        bad += ['%s: argument %d is `%s`, bound as %s' % (name, i, a, getattr(c, '__name__', c))
                for i, (a, c) in enumerate(zip(args, argtypes)) if not _arg_matches(a, c)]
    return bad


def test_ctypes_signatures_match_header_types():
    """Return type, argument count and every argument type of _hip.SIGNATURES against the header's prototypes: an
    int bound as c_int64, or a float bound as c_double, loads and runs and reads garbage."""
    from decomp_amd import _hip
    protos = _prototypes(open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read())
    names = [p[1] for p in protos]
    assert len(names) == len(set(names)) and set(names) == set(_declared()) == set(_hip.SIGNATURES)
    bad = _mismatches(protos, _hip.SIGNATURES)
    assert not bad, '\n'.join(bad)


def test_signature_check_rejects_wrong_and_unknown_types():
    sig = {'dcp_f': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_int)])}
    good = _prototypes('extern "C" {\nint dcp_f(dcp_handle* h, int n /* < 0: none */, float tol,\n int* it_out);\n}')
    assert good == [('int', 'dcp_f', ['dcp_handle* h', 'int n', 'float tol', 'int* it_out'])]
    assert _mismatches(good, sig) == []
    for arg, wrong in (('int n', 'int64_t n'), ('int n', 'unsigned n'), ('float tol', 'double tol'),
                       ('int* it_out', 'int64_t* it_out')):
        proto = [('int', 'dcp_f', [wrong if a == arg else a for a in good[0][2]])]
        assert len(_mismatches(proto, sig)) == 1, wrong
    assert len(_mismatches([('int64_t', 'dcp_f', good[0][2])], sig)) == 1
    assert len(_mismatches([('int', 'dcp_f', good[0][2][:3])], sig)) == 1
    with pytest.raises(AssertionError):
        _mismatches([('int', 'dcp_f', ['dcp_handle* h', 'size_t n', 'float tol', 'int* it_out'])], sig)
    with pytest.raises(AssertionError):
        _prototypes('extern "C" {\nstruct dcp_opts { int a; };\n}')


def test_build_info_and_error_paths_without_gpu():
    from decomp_amd import _hip
    lib = _hip.load()
    assert b'gfx950' in lib.dcp_build_info()
    # width of the all-reduced statistics (pure host arithmetic)
    assert lib.dcp_nmf_mu_stats_width(4096, 256, 0, 0) == 4096 + 256
    assert lib.dcp_nmf_mu_stats_width(4096, 256, 0, 1) == 8192
    assert lib.dcp_nmf_mu_stats_width(4096, 256, 1, 0) == 8192
    # null handle -> DCP_ERR_INVALID, never a crash
    assert lib.dcp_set_stream(None, None) == -1
    assert lib.dcp_profile_enable(None, 1) == -1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from decomp_amd import _hip
    monkeypatch.setattr(_hip, '_lib', None)
    monkeypatch.setattr(_hip, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_hip.HipLibraryError):
        _hip.load()
