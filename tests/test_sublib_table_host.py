"""The table of C-ABI libraries (quant/_sublibs.py) against the headers under include/ (no GPU, no built library): every
header function has a prototype and the reverse, with as many arguments as the declaration has parameters and a ctypes kind
per parameter that matches the C type; no two entries overlap; ``__graft_entry__.SUBLIBS`` and the public names of
``quant._hip`` are the table's."""

import ctypes
import os
import re

import pytest

from quant import _sublibs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
# (header, prototypes) of every library: the main one's two headers, then one per entry of the table
HEADERS = list(_sublibs.MAIN_PROTOTYPES.items()) + [(s.header, s.prototypes) for s in _sublibs.SUBLIBS]
BY_VALUE = {'float': (ctypes.c_float,), 'int64_t': (ctypes.c_int64,), 'long long': (ctypes.c_int64,),
            'size_t': (ctypes.c_size_t,), 'int': (ctypes.c_int, ctypes.c_int32), 'int32_t': (ctypes.c_int, ctypes.c_int32)}


def stripped(header):
    with open(os.path.join(INCLUDE, header)) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def declared_functions(header):
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', stripped(header))))


def declarations(header):
    """{function: (return type, [parameter, ...])} of the header: the parameter list is split at the commas at parenthesis
    depth 0, ``(void)`` and ``()`` are no parameters."""
    text, out = stripped(header), {}
    for m in re.finditer(r'^[ \t]*([A-Za-z_][\w \t\*]*?)[ \t]*\b(lsq_[a-z0-9_]+)\s*\(', text, flags=re.M):
        depth, params, start = 1, [], m.end()
        for pos in range(m.end(), len(text)):
            c = text[pos]
            depth += (c == '(') - (c == ')')
            if depth == 0 or (depth == 1 and c == ','):
                params.append(' '.join(text[start:pos].split()))
                start = pos + 1
            if depth == 0:
                break
        assert depth == 0 and text[pos + 1:].lstrip().startswith(';'), (header, m.group(2))
        assert m.group(2) not in out, (header, m.group(2))
        out[m.group(2)] = (' '.join(m.group(1).split()), [] if params in ([''], ['void']) else params)
    return out


def matches(c_type, ctype):
    """Whether the ctypes type can carry a value the header declares as ``c_type`` (a parameter without its name)."""
    if '*' in c_type:
        return ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer) or \
            (ctype is ctypes.c_char_p and c_type.replace(' ', '') == 'constchar*')
    return ctype in BY_VALUE.get(re.sub(r'\bconst\b', '', c_type).strip(), ())


def test_the_parser_reads_what_it_should():
    d = declarations('lsq_hip.h')
    assert d['lsq_abi_version'] == ('int', []) and d['lsq_error_string'] == ('const char*', ['int code'])
    assert d['lsq_solve_rows'][1][:3] == ['const float* rows', 'int64_t R', 'int64_t M'] and len(d['lsq_solve_rows'][1]) == 11
    assert matches('const float*', ctypes.c_void_p) and matches('const lsq_conv_geom*', ctypes.POINTER(_sublibs.ConvGeom))
    assert not matches('const float*', ctypes.c_int64) and not matches('float', ctypes.c_void_p)
    assert not matches('int64_t', ctypes.c_int) and not matches('int', ctypes.c_int64) and not matches('size_t', ctypes.c_int)
    assert matches('size_t', ctypes.c_size_t) and matches('long long', ctypes.c_int64) and matches('int32_t', ctypes.c_int)
    assert not matches('double', ctypes.c_float) and not matches('lsq_conv_geom', ctypes.c_void_p)


@pytest.mark.parametrize('header, prototypes', HEADERS, ids=[h for h, _ in HEADERS])
def test_the_prototypes_are_the_headers_declarations(header, prototypes):
    found = declarations(header)
    assert sorted(found) == declared_functions(header)               # (the parser missed no function of the header)
    assert sorted(prototypes) == sorted(found)
    for symbol, (restype, argtypes) in prototypes.items():
        c_return, params = found[symbol]
        assert matches(c_return, restype), (symbol, c_return, restype)
        assert len(argtypes) == len(params), (symbol, len(argtypes), params)
        for param, ctype in zip(params, argtypes):
            c_type = param if param.endswith('*') else re.sub(r'\s*\b\w+$', '', param)      # (without the parameter's name)
            assert matches(c_type, ctype), (symbol, param, ctype)


def test_every_entry_is_of_one_library_alone():
    subs = _sublibs.SUBLIBS
    for field in ('dir', 'header', 'version_symbol'):
        assert len({getattr(s, field) for s in subs}) == len(subs), field
    symbols = [sym for _, prototypes in HEADERS for sym in prototypes]
    assert len(set(symbols)) == len(symbols)
    assert _sublibs.BY_DIR == {s.dir: s for s in subs}
    for s in subs:
        assert next(iter(s.prototypes)) == s.version_symbol and s.prototypes[s.version_symbol] == (ctypes.c_int, [])
        assert all(re.fullmatch(s.pattern, sym) for sym in s.prototypes), s.dir
        define = re.findall(r'#define\s+LSQ_' + s.dir.upper() + r'_ABI_VERSION\s+(\d+)\b', stripped(s.header))
        assert define == [str(s.version)], s.header
        assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', s.dir, 'Makefile')), s.dir


def test_the_build_rows_and_the_public_names_are_the_tables():
    import __graft_entry__
    from quant import _hip
    assert re.findall(r'#define\s+LSQ_ABI_VERSION\s+(\d+)\b', stripped('lsq_hip.h')) == [str(_hip.ABI_VERSION)]
    assert len(__graft_entry__.SUBLIBS) == len(_sublibs.SUBLIBS) >= 12
    for row, s in zip(__graft_entry__.SUBLIBS, _sublibs.SUBLIBS):
        assert len(row) == 6 and row[0] == s.dir and row[2:4] == (s.header, s.pattern)
        assert row[4] == tuple(s.prototypes) and row[4][0] == s.version_symbol
        assert row[1] == s.dir + '_lib' and callable(getattr(_hip, row[1]))
        assert row[5] == s.dir.upper() + '_ABI_VERSION' and getattr(_hip, row[5]) == s.version
        path = getattr(_hip, s.dir + '_library_path')()
        assert path == os.path.join(ROOT, 'ml-quant_amd', 'lib', 'liblsq_hip_' + s.dir + '.so')
