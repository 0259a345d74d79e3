"""Call sites of the kernel library against its bindings, checked without a GPU.

The bindings take their signatures from csrc/pra_api.h and every argument is positional, so a
call with one argument too few or too many, or to a binding that is gone, would only show when
that line runs on a GPU. Here every call on the library under paddle_ray_amd/ is found with
``ast`` and held against the loaded module: the entry exists, the arguments are plain
positionals, and their number is the arity in the binding's pybind11 signature.

A use of the library handle that is not ``<handle>.<entry>(...)`` (returning it, passing it on,
a ``*args`` call) cannot be checked statically and fails the test instead of being left out.
"""
import ast
import os
import re

import pytest

from paddle_ray_amd.ops import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bindings with no caller in the repository, kept on purpose
UNCALLED_OK = {
    'adl_supported',    # the kernel's own column limit; ops/fused.py _adl_ok states the same rule
}


def _module():
    mod = _native._load()
    if mod is None:
        pytest.skip(f"library not loadable here: {_native.load_error()}")
    return mod


def _py_files(*dirs):
    for d in dirs:
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in sorted(files):
                if f.endswith('.py'):
                    yield os.path.join(base, f)


def _is_handle(node, in_native):
    """``_native.lib()`` / ``X._native.lib()`` (and a bare ``lib()`` inside _native.py)."""
    if not (isinstance(node, ast.Call) and not node.args and not node.keywords):
        return False
    f = node.func
    if isinstance(f, ast.Attribute) and f.attr == 'lib':
        v = f.value
        return (isinstance(v, ast.Name) and v.id == '_native') or \
               (isinstance(v, ast.Attribute) and v.attr == '_native')
    return in_native and isinstance(f, ast.Name) and f.id == 'lib'


def _scopes(tree):
    """The module body without its functions and classes' methods, then each outermost function
    (nested functions and lambdas belong to the function around them)."""
    outer = []

    def visit(node, top):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                outer.append(child)
            elif isinstance(child, ast.ClassDef):
                visit(child, top)
            else:
                top.append(child)
                visit(child, top)
    top = []
    visit(tree, top)
    return top, outer


def _sites(path):
    """([(lineno, entry, call node)], [unresolved uses]) of one file."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    in_native = os.path.basename(path) == '_native.py' and 'ops' in path
    rel = os.path.relpath(path, ROOT)
    parent = {c: p for p in ast.walk(tree) for c in ast.iter_child_nodes(p)}
    top_nodes, funcs = _scopes(tree)

    def bound_names(nodes):
        names, other = set(), set()
        for n in nodes:
            if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
                (names if _is_handle(n.value, in_native) else other).add(n.targets[0].id)
        return names, other

    module_names, _ = bound_names(top_nodes)
    sites, bad = [], []

    def check_use(expr, scope_desc):
        """expr evaluates to the library: it must be the receiver of ``.<entry>(...)``, the value
        of a plain ``name = ...`` binding, or a discarded expression statement."""
        p = parent.get(expr)
        if isinstance(p, ast.Attribute) and p.value is expr and isinstance(parent.get(p), ast.Call) \
                and parent[p].func is p:
            sites.append((p.lineno, p.attr, parent[p]))
        elif isinstance(p, ast.Assign) and p.value is expr and len(p.targets) == 1 \
                and isinstance(p.targets[0], ast.Name):
            pass
        elif isinstance(p, ast.Expr):
            pass
        else:
            bad.append(f"{rel}:{expr.lineno}: library handle used outside a direct call ({scope_desc})")

    def scan(nodes, names, scope_desc):
        for n in nodes:
            if _is_handle(n, in_native):
                check_use(n, scope_desc)
            elif isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and n.id in names:
                check_use(n, scope_desc)

    scan(top_nodes, module_names, 'module level')
    for fn in funcs:
        nodes = list(ast.walk(fn))
        names, other = bound_names(nodes)
        for clash in sorted(names & other):
            bad.append(f"{rel}:{fn.lineno}: {fn.name} binds {clash} to the library and to something else")
        # a parameter or other binding of the same name hides a module-level handle
        hidden = other | {a.arg for n in nodes if isinstance(n, ast.arguments)
                          for a in n.args + n.kwonlyargs + n.posonlyargs}
        scan(nodes, names | (module_names - hidden), fn.name)
    return sites, bad


def _arity(fn):
    """Number of parameters in the pybind11 signature line of a bound function."""
    sig = fn.__doc__.splitlines()[0]
    assert sig.startswith(fn.__name__ + '(') and ') -> ' in sig, sig
    return len(re.findall(r'\barg\d+: ', sig))


def _all_sites():
    sites, bad = [], []
    for path in _py_files('paddle_ray_amd'):
        s, b = _sites(path)
        sites += [(os.path.relpath(path, ROOT), *x) for x in s]
        bad += b
    return sites, bad


def test_every_library_call_matches_its_binding():
    mod = _module()
    sites, bad = _all_sites()
    assert len(sites) >= 50, f"only {len(sites)} call sites found: the scan lost the library handle"
    for rel, line, entry, call in sites:
        where = f"{rel}:{line}: {entry}"
        fn = getattr(mod, entry, None)
        if fn is None:
            bad.append(f"{where}: no such binding")
            continue
        if call.keywords or any(isinstance(a, ast.Starred) for a in call.args):
            bad.append(f"{where}: keyword or starred arguments (the bindings are positional)")
        elif len(call.args) != _arity(fn):
            bad.append(f"{where}: {len(call.args)} arguments, the binding takes {_arity(fn)}")
    assert not bad, '\n'.join(bad)


def test_every_binding_has_a_caller():
    mod = _module()
    called = set()
    for path in _py_files('paddle_ray_amd', 'scripts', 'tests'):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        called |= {n.func.attr for n in ast.walk(tree)
                   if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
    public = {n for n in dir(mod) if not n.startswith('_') and callable(getattr(mod, n))}
    assert len(public) > 60, sorted(public)
    stale = sorted(public - called - UNCALLED_OK)
    assert not stale, f"bindings nobody calls (remove them or list them in UNCALLED_OK): {stale}"
    assert not sorted(UNCALLED_OK - public), "UNCALLED_OK names a binding that is gone"


def test_scan_flags_what_it_cannot_resolve(tmp_path):
    """The scan itself: direct and bound calls are found, anything else is reported."""
    src = ("from paddle_ray_amd.ops import _native\n"
           "def a(x):\n"
           "    L = _native.lib()\n"
           "    L.colsum(x, 1)\n"
           "    return _native.lib().zero_mt(x)\n"
           "def b():\n"
           "    return _native.lib()\n"
           "def c(f):\n"
           "    L = _native.lib()\n"
           "    f(L)\n")
    p = tmp_path / 'm.py'
    p.write_text(src)
    sites, bad = _sites(str(p))
    assert [(line, entry, len(call.args)) for line, entry, call in sites] == [(4, 'colsum', 2), (5, 'zero_mt', 1)]
    assert len(bad) == 2 and ':7:' in bad[0] and ':10:' in bad[1], bad
