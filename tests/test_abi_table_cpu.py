"""The ctypes prototype table (``brainevent_amd/_abi.py``) against the public header, and ``_lib.fn`` on top of it.

A new entry point needs its declaration in ``include/brainevent_amd.h`` and one line in the table; these tests hold the two
together and keep the package's call sites on the table.  No GPU: nothing here launches a kernel."""
import ast
import ctypes
import itertools
import os
import re
import subprocess

import pytest

from brainevent_amd import _abi, _lib
from brainevent_amd._error import KernelExecutionError, KernelLoadError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'brainevent_amd.h')
PKG = os.path.join(ROOT, 'brainevent_amd')

_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32, 'double': ctypes.c_double}
#: what a ``POINTER(T)`` may point at, by the header's pointee
_POINTEES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
             'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float}


def _c_type(text):
    """A declared type as ``'int'`` / ``'int64_t'`` / ``'uint32_t'`` / ``'double'`` or ``('*', pointee)``; ``be_stream_t`` is
    ``void*`` and a pointer to a pointer has the pointee ``'*'``."""
    text = re.sub(r'\bconst\b', ' ', text).strip()
    if text == 'be_stream_t':
        return ('*', 'void')
    if '*' in text:
        base, stars = text.replace('*', ' ').split(), text.count('*')
        assert len(base) == 1, text
        return ('*', base[0] if stars == 1 else '*')
    assert text in _SCALARS, text
    return text


def header_prototypes():
    """name -> (return type, [argument types]) of every function the header declares, after macro expansion."""
    src = subprocess.run(['gcc', '-E', '-P', HEADER], check=True, capture_output=True, text=True).stdout
    protos = {}
    for ret, name, args in re.findall(r'((?:const\s+)?\w+\s*\*?)\s*\b(be_\w+)\s*\(([^()]*)\)\s*;', src):
        assert name not in protos, name
        args = [] if args.strip() == 'void' else [re.sub(r'\w+\s*$', '', a) for a in args.split(',')]     # drop the names
        protos[name] = (_c_type(ret), [_c_type(a) for a in args])
    return protos


def _agrees(ct, c, is_return=False):
    if isinstance(c, str):
        return ct is _SCALARS[c]
    if is_return:
        return c == ('*', 'char') and ct is ctypes.c_char_p
    if ct is ctypes.c_void_p:
        return True
    if isinstance(ct, type) and issubclass(ct, ctypes._Pointer):
        return ct._type_ is (ctypes.c_void_p if c[1] == '*' else _POINTEES.get(c[1]))
    return False


def mismatches(table, header):
    """Every disagreement between a prototype table and the header's prototypes, as text (empty: they agree)."""
    out = [f'{n}: declared, not in the table' for n in sorted(set(header) - set(table))]
    out += [f'{n}: in the table, not declared' for n in sorted(set(table) - set(header))]
    for name in sorted(set(table) & set(header)):
        (restype, argtypes), (c_ret, c_args) = table[name], header[name]
        if not _agrees(restype, c_ret, is_return=True):
            out.append(f'{name}: returns {c_ret}, table says {restype}')
        if len(argtypes) != len(c_args):
            out.append(f'{name}: {len(c_args)} arguments, table has {len(argtypes)}')
            continue
        out += [f'{name}: argument {i} is {c}, table says {ct}' for i, (ct, c) in enumerate(zip(argtypes, c_args))
                if not _agrees(ct, c)]
    return out


@pytest.fixture(scope='module')
def header():
    return header_prototypes()


def test_table_matches_header(header):
    assert len(header) >= 321
    rets = {r for r, _ in header.values()}
    assert rets == {'int', 'int64_t', ('*', 'char')}, rets
    assert set(_abi.PROTOTYPES) == set(header)
    assert mismatches(_abi.PROTOTYPES, header) == []


def test_the_comparison_can_fail(header):
    name = 'be_binary_csrmv_t_binned'
    restype, argtypes = _abi.PROTOTYPES[name]
    assert argtypes[10] is ctypes.c_int64
    wrong_type = argtypes[:10] + (ctypes.c_int,) + argtypes[11:]
    for bad, what in (((restype, wrong_type), 'argument 10'), ((restype, argtypes[:-1]), '18 arguments, table has 17'),
                      ((ctypes.c_int64, argtypes), 'returns int')):
        found = mismatches({**_abi.PROTOTYPES, name: bad}, header)
        assert len(found) == 1 and found[0].startswith(name) and what in found[0], found
    # a typed pointer has to point at what the header says; a scalar is not a pointer; a missing / extra name shows
    typed = {**_abi.PROTOTYPES, 'be_profile_read': (ctypes.c_int, (ctypes.POINTER(ctypes.c_int), ctypes.c_int))}
    assert len(mismatches(typed, header)) == 1
    scalar = {**_abi.PROTOTYPES, 'be_profile_read': (ctypes.c_int, (ctypes.c_int64, ctypes.c_int))}
    assert len(mismatches(scalar, header)) == 1
    fewer = {k: v for k, v in _abi.PROTOTYPES.items() if k != name}
    assert mismatches(fewer, header) == [f'{name}: declared, not in the table']
    assert mismatches({**_abi.PROTOTYPES, 'be_extra': (ctypes.c_int, ())}, header) == ['be_extra: in the table, not declared']


# ---------------------------------------------------------------------------------------------------------------------------
# call sites of the package
# ---------------------------------------------------------------------------------------------------------------------------
#: the values a placeholder of an f-string symbol name ranges over (the header's naming grammar)
FAMILIES = [{'s', 'u', 'n'}, {'mv', 'mm'}, {'trans', 'notrans'}, {'f32', 'f64', 'f16', 'bf16'}, {'bool', 'float'},
            {'t', 'nt'}, {'homo', 'hetero'}, {'scatter', 'gather'}, {'transpose', 'no_transpose'}]
_ANY = '(' + '|'.join(sorted({v for f in FAMILIES for v in f}, key=len, reverse=True)) + ')'


def _symbol_names(node, assigned):
    """The symbol names an expression at a call site can stand for: literals as they are, an f-string as the table's names it
    matches (checked to be a full product of families), a conditional as both arms, a local variable as what it was assigned."""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return [node.value]
    if isinstance(node, ast.IfExp):
        return _symbol_names(node.body, assigned) + _symbol_names(node.orelse, assigned)
    if isinstance(node, ast.Name) and node.id in assigned:
        return [n for v in assigned[node.id] for n in _symbol_names(v, assigned)]
    if isinstance(node, ast.JoinedStr):
        pattern = ''.join(re.escape(p.value) if isinstance(p, ast.Constant) else _ANY for p in node.values)
        found = {m.groups() for m in (re.fullmatch(pattern, n) for n in _abi.PROTOTYPES) if m}
        assert found, f'no declared symbol matches {ast.unparse(node)}'
        columns = [set(c) for c in zip(*found)]
        assert all(c in FAMILIES for c in columns), (ast.unparse(node), columns)
        assert found == set(itertools.product(*columns)), f'{ast.unparse(node)}: some expansion is not declared'
        return [n for n in _abi.PROTOTYPES if re.fullmatch(pattern, n)]
    raise AssertionError(f'symbol name not resolvable: {ast.unparse(node)}')


def _own_nodes(scope):
    """The nodes of a function (or module) without those of the functions defined inside it."""
    todo = list(ast.iter_child_nodes(scope))
    while todo:
        n = todo.pop()
        yield n
        if not isinstance(n, ast.FunctionDef):
            todo.extend(ast.iter_child_nodes(n))


def _call_sites():
    """(file, line, names) of every ``fn(...)`` / ``call(...)`` of ``_lib`` in the package; asserts the one-argument ``fn``."""
    sites = []
    for fname in sorted(os.listdir(PKG)):
        if not fname.endswith('.py') or fname == '_lib.py':
            continue
        tree = ast.parse(open(os.path.join(PKG, fname)).read())
        imported = {a.asname or a.name for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.module == '_lib'
                    for a in n.names} & {'fn', 'call'}
        for scope in ast.walk(tree):
            if not isinstance(scope, (ast.Module, ast.FunctionDef)):
                continue
            nodes = list(_own_nodes(scope))
            assigned = {}
            for n in nodes:
                if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
                    assigned.setdefault(n.targets[0].id, []).append(n.value)
            for n in nodes:
                f = n.func if isinstance(n, ast.Call) else None
                if isinstance(f, ast.Name) and f.id in imported:
                    which = f.id
                elif isinstance(f, ast.Attribute) and f.attr in ('fn', 'call') and ast.unparse(f.value) == '_lib':
                    which = f.attr
                else:
                    continue
                assert n.args, (fname, n.lineno)
                if which == 'fn':
                    assert len(n.args) == 1 and not n.keywords, f'{fname}:{n.lineno}: fn() takes the name alone in the package'
                sites.append((fname, n.lineno, _symbol_names(n.args[0], assigned)))
    return sites


def test_every_call_site_of_the_package_is_in_the_table():
    sites = _call_sites()
    assert len({(f, l) for f, l, _ in sites}) >= 80, len(sites)
    for fname, line, names in sites:
        assert names and all(n in _abi.PROTOTYPES for n in names), (fname, line, names)
    used = {n for _, _, names in sites for n in names}
    assert {'be_binary_jitnmm_trans_bf16', 'be_binary_csrmm_nt_indexed', 'be_dt2t', 'be_grad_rows', 'be_plasticity_rows',
            'be_lif_step_scaled_packed', 'be_scatter_plan_patch_entries', 'be_csrmm'} <= used


def test_package_has_no_prototype_lists_left():
    for fname in sorted(os.listdir(PKG)):
        if fname.endswith('.py') and fname not in ('_lib.py', '_abi.py'):
            src = open(os.path.join(PKG, fname)).read()
            assert not re.search(r'\bargtypes\b|\brestype\b', src), fname


# ---------------------------------------------------------------------------------------------------------------------------
# _lib.fn
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built():
    if _lib.needs_build():
        _lib.build()


def test_fn_sets_the_table_prototype(built):
    for name in ('be_binary_csrmv_t_binned', 'be_binned_bins', 'be_binary_csrmv_t_binned_workspace_bytes', 'be_last_error',
                 'be_build_arch', 'be_weight_stats'):
        f = _lib.fn(name)
        restype, argtypes = _abi.PROTOTYPES[name]
        assert f.restype is restype and tuple(f.argtypes) == argtypes
        assert _lib.fn(name) is f
    assert _lib.fn('be_build_arch')() == b'gfx950'
    assert _lib.lib().be_last_error.restype is ctypes.c_char_p


def test_fn_refuses_an_undeclared_symbol(built):
    with pytest.raises(KernelLoadError, match='be_no_such_symbol'):
        _lib.fn('be_no_such_symbol')
    with pytest.raises(KernelLoadError, match='be_no_such_symbol'):
        _lib.fn('be_no_such_symbol', ctypes.c_int, [ctypes.c_int])


def test_fn_checks_a_list_it_is_given(built):
    i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    f = _lib.fn('be_exchange_slice_for')
    typed = [i64, ci, ci] + [ctypes.POINTER(i64)] * 3
    assert _lib.fn('be_exchange_slice_for', ci, typed) is f
    assert _lib.fn('be_exchange_slice_for', ci, [i64, ci, ci, vp, vp, vp]) is f              # pointer flavour does not matter
    assert _lib.fn('be_exchange_slice_for', argtypes=[i64, ci, ci, vp, ctypes.POINTER(ctypes.c_float), vp]) is f
    assert tuple(f.argtypes) == _abi.PROTOTYPES['be_exchange_slice_for'][1]                  # ... and none of them was installed
    assert _lib.fn('be_profile_read', ci, [vp, ci]) is _lib.fn('be_profile_read')            # (bench.py's form)
    with pytest.raises(TypeError, match=r'be_exchange_slice_for.*argument 1'):
        _lib.fn('be_exchange_slice_for', ci, [i64, i64, ci, vp, vp, vp])
    with pytest.raises(TypeError, match=r'be_exchange_slice_for.*argument 3'):
        _lib.fn('be_exchange_slice_for', ci, [i64, ci, ci, i64, vp, vp])                     # a scalar where a pointer goes
    with pytest.raises(TypeError, match=r'be_exchange_slice_for.*5 arguments'):
        _lib.fn('be_exchange_slice_for', ci, [i64, ci, ci, vp, vp])
    with pytest.raises(TypeError, match=r'be_exchange_slice_for.*return'):
        _lib.fn('be_exchange_slice_for', i64, typed)
    with pytest.raises(TypeError, match='be_exchange_slice_for'):                            # every time, not only the first
        _lib.fn('be_exchange_slice_for', ci, [i64, i64, ci, vp, vp, vp])


def test_call_checks_the_status(built):
    lo, hi, words = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib.call('be_exchange_slice_for', 100, 2, 1, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(words)) is None
    assert 0 < lo.value < hi.value == 100
    # a negative status (BE_ERR_INVALID; the library refuses before it stores anything): the symbol and be_last_error's text
    with pytest.raises(KernelExecutionError, match=r'be_binned_set_tuning: status -\d+: .*task_groups and min_tasks must be >= 1'):
        _lib.call('be_binned_set_tuning', 0, 0)
    assert 'must be >= 1' in _lib.last_error()
    with pytest.raises(ctypes.ArgumentError):
        _lib.call('be_binned_set_tuning', 256, 'x')
