"""Lower the SymPy stencil IR of a Model to the per-node C bodies that the
hand-written kernel skeleton (csrc/tf_kernels.h) is specialised with.

The reference hands ``model.F_array`` / ``model._J_sparse_array`` to
``sympy.lambdify`` and lets NumPy evaluate the printed expression
(``triflow/core/compilers.py:207-219``).  To compute *the same floating-point
values*, this lowering starts from the very string SymPy's NumPy printer
produces for that call, parses it with ``ast`` and emits C with the identical
operation tree (no re-association, no common-subexpression rewriting, no FMA
contraction; the C compiler may only share bit-identical subtrees).  Name
overrides follow the reference's module dictionary: ``Heaviside`` is
identically one (``compilers.py:204-205``), ``Max``/``Min`` are
``numpy.maximum``/``minimum`` chains.  A model built with ``heaviside="exact"``
opts out of the first: ``Heaviside`` is ``numpy.heaviside``, ``DiracDelta`` zero,
``Piecewise`` ``numpy.select``.
"""

import ast
import hashlib
import inspect
import os

import numpy as np
from sympy import lambdify

_FUNCS_1 = {"sqrt": "sqrt", "exp": "exp", "log": "log", "sin": "sin", "cos": "cos",
            "tan": "tan", "tanh": "tanh", "sinh": "sinh", "cosh": "cosh",
            "arctan": "atan", "arcsin": "asin", "arccos": "acos",
            "abs": "tf_abs", "absolute": "tf_abs", "fabs": "tf_abs", "sign": "tf_sign",
            "log10": "log10", "log2": "log2", "cbrt": "cbrt", "expm1": "expm1",
            "log1p": "log1p", "floor": "floor", "ceil": "ceil"}


class UnsupportedExpression(NotImplementedError):
    pass


#: the two meanings of the discontinuous vocabulary (``Model(..., heaviside=...)``):
#: "one" -- every Heaviside is the literal 1.0, as in the reference's module dictionary; DiracDelta and
#: Piecewise are refused.  "exact" -- Heaviside is numpy.heaviside, DiracDelta is zero, Piecewise is
#: numpy.select.
HEAVISIDE_MODES = ("one", "exact")

_EXACT_HINT = '; Model(..., heaviside="exact") lowers Heaviside, DiracDelta and Piecewise exactly'


def _dirac_zero(a, *_):
    return np.zeros_like(a)


#: what SymPy's lambdify is given for the names NumPy does not define, per mode: the printed call keeps
#: the name, and this is its meaning
LAMBDIFY_MODULES = {
    "one": [{"Heaviside": lambda *a: 1}, "numpy"],
    "exact": [{"Heaviside": np.heaviside, "DiracDelta": _dirac_zero}, "numpy"],
}


def validate_heaviside(mode):
    """The one validator of the setting (Model, hip_compiler and the lowering all come here)."""
    if mode not in HEAVISIDE_MODES:
        raise ValueError("heaviside=%r: expected one of %s" % (mode, ", ".join(map(repr, HEAVISIDE_MODES))))
    return mode


def heaviside_mode(model):
    """The one place the lowering reads the mode from: the model's ``_heaviside`` (a foreign model
    without the attribute is in the default mode; ``hip_compiler(model, heaviside=...)`` sets it)."""
    return validate_heaviside(getattr(model, "_heaviside", "one"))


_COMPARE = {"greater": ">", "greater_equal": ">=", "less": "<", "less_equal": "<=", "equal": "==",
            "not_equal": "!="}


def _dbl(value):
    """C literal with the exact binary value of a Python number."""
    f = float(value)
    if f != value and not isinstance(value, float):
        raise UnsupportedExpression("integer constant %r is not a double" % (value,))
    if f == int(f) and abs(f) < 2 ** 53:
        return "%d.0" % int(f)
    return f.hex()          # C99 / C++17 hexadecimal floating literal


class _CEmitter(ast.NodeVisitor):
    """Python expression AST -> C expression string.  Also tracks which
    sub-expressions are *uniform* (same value for every node a thread visits:
    dx, scalar parameters, constants) so that divisions by a uniform divisor can
    use the exact reciprocal form ``tf_div_u`` with the divisor and its
    reciprocal hoisted out of the node loop."""

    def __init__(self, names, uniform_names=(), heaviside="one"):
        self.names = names          # python identifier -> C expression
        self.exact = heaviside == "exact"
        self.uniform_names = set(uniform_names)
        self.denominators = {}      # C expression -> index
        self.den_count = {}         # C expression -> number of quotients using it
        self.shared = {}            # den_count of a previous pass over the same expressions
        self.host_consts = {}       # python source of a uniform pow()/libm call -> index

    def host_const(self, node):
        """A node-independent power or libm call (``dx**3``, ``exp(k)``): evaluated on
        the host with NumPy -- i.e. by the very libm the reference's lambdified code
        calls -- and handed to the kernel as an extra scalar, so its bits match."""
        src = ast.unparse(node)
        k = self.host_consts.setdefault(src, len(self.host_consts))
        return "tf_hc[%d]" % k

    def is_uniform(self, node):
        if isinstance(node, ast.Constant):
            return True
        if isinstance(node, ast.Name):
            return node.id in self.uniform_names or node.id in ("pi", "E", "e")
        if isinstance(node, ast.UnaryOp):
            return self.is_uniform(node.operand)
        if isinstance(node, ast.BinOp):
            return self.is_uniform(node.left) and self.is_uniform(node.right)
        if isinstance(node, ast.Call):
            args = []
            for a in node.args:
                args.extend(a.elts if isinstance(a, (ast.List, ast.Tuple)) else [a])
            return all(self.is_uniform(a) for a in args
                       if not isinstance(a, (ast.Name, ast.Attribute)) or
                       not (getattr(a, "id", getattr(a, "attr", "")) in ("maximum", "minimum")))
        return False

    def visit_Name(self, node):
        if node.id in self.names:
            return self.names[node.id]
        if node.id == "pi":
            return _dbl(np.pi)
        if node.id in ("E", "e"):           # SymPy's Euler number, printed as numpy.e
            return _dbl(np.e)
        raise UnsupportedExpression("unknown symbol %r in stencil expression" % node.id)

    def visit_Constant(self, node):
        if isinstance(node.value, bool) or not isinstance(node.value, (int, float)):
            raise UnsupportedExpression("constant %r" % (node.value,))
        return _dbl(node.value)

    def visit_UnaryOp(self, node):
        operand = self.visit(node.operand)
        if isinstance(node.op, ast.USub):
            return "(-%s)" % operand
        if isinstance(node.op, ast.UAdd):
            return operand
        raise UnsupportedExpression(ast.dump(node))

    def visit_BinOp(self, node):
        if isinstance(node.op, ast.Pow):
            return self._pow(node)
        if isinstance(node.op, ast.Div) and not self.is_uniform(node.left):
            den = self.visit(node.right)
            self.den_count[den] = self.den_count.get(den, 0) + 1
            # uniform divisor: reciprocal hoisted out of the node loop; a
            # node-dependent divisor shared by several quotients of the same node:
            # one true division for the reciprocal, then the exact 3-op quotient
            if self.is_uniform(node.right) or self.shared.get(den, 0) >= 2:
                k = self.denominators.setdefault(den, len(self.denominators))
                # (exact mode: its states may be infinite where a step function keeps them out of the
                # result, and a tie of Max(U, 0) is a zero numerator whose sign counts; tf_div_x is
                # tf_div_u with IEEE's quotient for a non-finite or zero numerator)
                return "%s(%s, tf_den%d, tf_rden%d)" % ("tf_div_x" if self.exact else "tf_div_u",
                                                        self.visit(node.left), k, k)
        ops = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*", ast.Div: "/"}
        for klass, sym in ops.items():
            if isinstance(node.op, klass):
                return "(%s %s %s)" % (self.visit(node.left), sym, self.visit(node.right))
        raise UnsupportedExpression(ast.dump(node))

    def _pow(self, node):
        if self.is_uniform(node) and not isinstance(node.left, ast.Constant):
            return self.host_const(node)
        base = self.visit(node.left)
        expo = node.right
        neg = False
        if isinstance(expo, ast.UnaryOp) and isinstance(expo.op, ast.USub):
            neg, expo = True, expo.operand
        if isinstance(expo, ast.Constant) and isinstance(expo.value, (int, float)) \
                and not isinstance(expo.value, bool):
            val = -expo.value if neg else expo.value
            if val == 2:
                return "tf_sq(%s)" % base          # numpy.power fast path: square
            if val == 0.5:
                return "sqrt(%s)" % base           # numpy.power fast path: sqrt
            if val == 1:
                return base
            if val == -1:
                return "(1.0 / %s)" % base         # numpy.power fast path: reciprocal
            if float(val) == int(val) and abs(val) <= 16:
                return "tf_powi(%s, %d)" % (base, int(val))
            return "pow(%s, %s)" % (base, _dbl(val))
        return "pow(%s, %s)" % (base, self.visit(node.right))

    def visit_Call(self, node):
        name = node.func.attr if isinstance(node.func, ast.Attribute) else node.func.id
        if name == "Heaviside":
            if not self.exact:
                return "1.0"                       # reference compilers.py:204-205
            if len(node.args) not in (1, 2) or node.keywords:
                raise UnsupportedExpression("Heaviside with %d arguments" % len(node.args))
            # SymPy prints the value at zero; a one-argument call (older SymPy) means 1/2
            h0 = self.visit(node.args[1]) if len(node.args) == 2 else "0.5"
            return "tf_heaviside(%s, %s)" % (self.visit(node.args[0]), h0)
        if name == "DiracDelta" and self.exact:
            # only ever the derivative of a Heaviside of the state: the mass at the kink is dropped, as
            # SymPy drops it when it differentiates a Piecewise (the arguments are still checked)
            for a in node.args:
                self.visit(a)
            return "0.0"
        if name == "select" and self.exact:
            return self._select(node)
        if name == "reduce" and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) \
                and node.func.value.id in ("logical_and", "logical_or"):
            name = node.func.value.id               # (refused below, as greater / less ... are)
        if name == "reduce":                       # reduce(maximum, [a, b, ...])
            op = node.args[0]
            opname = op.attr if isinstance(op, ast.Attribute) else op.id
            fn = {"maximum": "tf_max", "minimum": "tf_min"}.get(opname)
            if fn is None or not isinstance(node.args[1], (ast.List, ast.Tuple)):
                raise UnsupportedExpression("reduce(%s, ...)" % opname)
            items = [self.visit(e) for e in node.args[1].elts]
            out = items[0]
            for item in items[1:]:
                out = "%s(%s, %s)" % (fn, out, item)
            return out
        if name in ("amax", "amin"):               # older SymPy: amax((a, b), axis=0)
            fn = "tf_max" if name == "amax" else "tf_min"
            items = [self.visit(e) for e in node.args[0].elts]
            out = items[0]
            for item in items[1:]:
                out = "%s(%s, %s)" % (fn, out, item)
            return out
        if name in ("maximum", "minimum"):
            fn = "tf_max" if name == "maximum" else "tf_min"
            return "%s(%s, %s)" % (fn, self.visit(node.args[0]), self.visit(node.args[1]))
        if name in _FUNCS_1 and len(node.args) == 1:
            if self.is_uniform(node.args[0]) and not isinstance(node.args[0], ast.Constant) \
                    and name not in ("abs", "absolute", "fabs", "sign", "floor", "ceil", "sqrt"):
                return self.host_const(node)
            return "%s(%s)" % (_FUNCS_1[name], self.visit(node.args[0]))
        if self.exact and (name in _COMPARE or name in ("logical_not", "logical_and", "logical_or")):
            raise UnsupportedExpression("function %r is only supported as a condition of Piecewise, not as a value"
                                        % name)
        hint = _EXACT_HINT if not self.exact and name in ("select", "DiracDelta") else ""
        raise UnsupportedExpression("function %r is not supported by the HIP compiler%s" % (name, hint))

    def _select(self, node):
        """``select([c1, c2, ...], [v1, v2, ...], default=nan)``, SymPy's print of a Piecewise: the first
        true condition wins, the default if none is.  A chain of tf_select, whose arguments are all
        evaluated, as NumPy evaluates every branch: the value is one of theirs, bit for bit."""
        if len(node.args) != 2 or not all(isinstance(a, (ast.List, ast.Tuple)) for a in node.args) \
                or len(node.args[0].elts) != len(node.args[1].elts) or not node.args[0].elts \
                or [k.arg for k in node.keywords] not in ([], ["default"]):
            raise UnsupportedExpression("unexpected form of select: " + ast.unparse(node))
        out = "tf_nan()"
        if node.keywords:
            d = node.keywords[0].value
            out = "tf_nan()" if isinstance(d, ast.Name) and d.id == "nan" else self.visit(d)
        for cond, value in reversed(list(zip(node.args[0].elts, node.args[1].elts))):
            out = "tf_select(%s, %s, %s)" % (self._cond(cond), self.visit(value), out)
        return out

    def _cond(self, node):
        """A condition of a Piecewise, as the NumPy printer writes Gt, Ge, Lt, Le, Eq, Ne, And, Or, Not and
        the literals -> a C bool with the same IEEE meaning (every comparison with a NaN is false,
        ``!=`` is true)."""
        if isinstance(node, ast.Constant) and isinstance(node.value, bool):
            return "true" if node.value else "false"
        if isinstance(node, ast.Call) and not node.keywords:
            f = node.func
            name = f.attr if isinstance(f, ast.Attribute) else getattr(f, "id", None)
            if name in _COMPARE and len(node.args) == 2:
                return "(%s %s %s)" % (self.visit(node.args[0]), _COMPARE[name], self.visit(node.args[1]))
            if name == "logical_not" and len(node.args) == 1:
                return "(!%s)" % self._cond(node.args[0])
            if name == "reduce" and isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) \
                    and f.value.id in ("logical_and", "logical_or") and len(node.args) == 1 \
                    and isinstance(node.args[0], (ast.List, ast.Tuple)) and node.args[0].elts:
                # (& and | of bools, not && and ||: nothing to short-circuit, so nothing to branch on)
                op = " & " if f.value.id == "logical_and" else " | "
                return "(%s)" % op.join(self._cond(e) for e in node.args[0].elts)
        raise UnsupportedExpression("condition %r of a Piecewise is not supported by the HIP compiler"
                                    % ast.unparse(node))

    def generic_visit(self, node):
        raise UnsupportedExpression(ast.dump(node))


def _printed_expressions(symbolic_args, exprs, heaviside="one"):
    """The element expressions of the list SymPy's lambdify would evaluate."""
    if not exprs:
        return []
    func = lambdify(symbolic_args, exprs, modules=LAMBDIFY_MODULES[heaviside],
                    cse=False)
    src = inspect.getsource(func)
    tree = ast.parse(src)
    fdef = tree.body[0]
    ret = fdef.body[-1]
    if len(fdef.body) != 1 or not isinstance(ret, ast.Return) \
            or not isinstance(ret.value, (ast.List, ast.Tuple)):
        raise UnsupportedExpression("unexpected lambdify output:\n" + src)
    return list(ret.value.elts)


def _c_ident(name):
    return "v_" + "".join(ch if ch.isalnum() else "_" for ch in name)


def _stencil_names(fields, pars, mp, parvec_mask):
    """python identifier (as printed by SymPy) -> C identifier, the declarations that read them from the
    register window / parameter array, and the names that are the same at every node."""
    names = {}
    decls = []
    for f, name in enumerate(fields):
        for off in range(-mp, mp + 1):
            key = name if off == 0 else "%s_%s%d" % (name, "m" if off < 0 else "p", abs(off))
            names[key] = _c_ident(key)
            decls.append("const double %s = w[%d][%d];" % (_c_ident(key), f, off + mp))
    for k, name in enumerate(pars):
        names[name] = _c_ident(name)
        decls.append("const double %s = par[%d];" % (_c_ident(name), k))
    names["dx"] = "dx"
    names["x"] = "xc"
    uniform = {"dx"} | {name for k, name in enumerate(pars) if not (parvec_mask >> k) & 1}
    return names, decls, uniform


def block_mask(nvar, pat_eq, pat_var):
    """``mask[eq][var]``: the entries of an nvar x nvar block of the banded solver that can be non-zero.

    The Jacobian pattern, united over the stencil offsets and with the diagonal added (A = I - c J),
    is a relation G on the variables; the patterns inside its reflexive-transitive closure G* are
    closed under sums, products and inverses, so every block the elimination forms lies in G*
    (DESIGN.md section 4).  ``TRIFLOW_BLOCK_MASK=0`` gives the all-true mask: the dense code, for
    A/B runs.  The mask is part of the generated header, so the caches keyed by it follow."""
    if os.environ.get("TRIFLOW_BLOCK_MASK", "1") == "0":
        return [[True] * nvar for _ in range(nvar)]
    m = [[r == c for c in range(nvar)] for r in range(nvar)]
    for e, v in zip(pat_eq, pat_var):
        m[e][v] = True
    for k in range(nvar):                           # Warshall
        for r in range(nvar):
            if m[r][k]:
                for c in range(nvar):
                    if m[k][c]:
                        m[r][c] = True
    return m


#: widest block ``mp * nvar`` whose level-1 walks hold their working set in registers: the bound of the
#: twisted walks (``tf_twist_h`` in csrc/tf_kernels.h carries the same 6) and of the factored outermost U block
REGISTER_BLOCK_MAX = 6


def outer_u_form(nvar, mp, pat_eq, pat_var, pat_off, j_uniform, j_alias, blk_nz):
    """The factored form of the outermost block of the stored pivot rows U~.

    The elimination never touches a row's outermost block, so ``U~[mp-1] = Dinv A(j, j +- mp)`` with
    ``A(j, j +- mp) = -c J(j, j +- mp)`` as the value table gives it: the level-1 walks can store
    the columns ``Dinv[:, S]`` instead, S = the equations that reach offset ``+-mp`` at all, and the
    back-substitution rebuilds the block from them and the Jacobian planes.  Per direction (index 0:
    offset ``+mp``, the down walk; index 1: ``-mp``, the up walk) this gives the pattern of the outer
    block, S, and the value planes to load (a proportional entry counts as the plane it aliases, a
    node-independent one is evaluated).  Returns None unless, for both directions,

        (entries of Dinv[:, S] inside the block mask) + (planes loaded)
            < (entries of the outer U~ block inside the block mask)

    -- or if ``TRIFLOW_U_OUTER=0`` asks for the stored form (A/B runs).  Scalar models exchange rows
    (the invariant does not hold) and never qualify: 1 + 0 < 1 is false.  Blocks too wide for the
    registers (``mp * nvar > REGISTER_BLOCK_MAX``, the bound of the twisted walks, tf_twist_h) keep the stored form as
    well: their walks spill already, and the columns of Dinv held for the store and the rebuilt block
    cost registers (wide4, 13 < 16 by the count: tfk_l1_factor_rhs 112 -> 132 bytes of scratch,
    tfk_l1_backsub_u occupancy 4 -> 3)."""
    if os.environ.get("TRIFLOW_U_OUTER", "1") == "0" or nvar < 2 or mp * nvar > REGISTER_BLOCK_MAX:
        return None
    nnz = len(pat_eq)
    form = dict(nz=[], rows=[], planes=[])
    for off in (mp, -mp):
        ks = [k for k in range(nnz) if pat_off[k] == off]
        nz = [[False] * nvar for _ in range(nvar)]
        for k in ks:
            nz[pat_eq[k]][pat_var[k]] = True
        rows = [any(nz[e]) for e in range(nvar)]
        planes = sorted({(j_alias[k] if j_alias[k] >= 0 else k) for k in ks if not j_uniform[k]})
        stored = sum(1 for r in range(nvar) for k in range(nvar) if rows[k] and blk_nz[r][k])
        block = sum(1 for r in range(nvar) for c in range(nvar) if blk_nz[r][c])
        if not stored + len(planes) < block:
            return None
        form["nz"].append(nz)
        form["rows"].append(rows)
        form["planes"].append(planes)
    return form


def _outer_u_lines(form, nvar, nnz):
    """The header lines of outer_u_form (none for a model that keeps the stored form)."""
    if form is None:
        return []

    def bools(values):
        return "{%s}" % ", ".join("true" if v else "false" for v in values)
    return [
        "// outermost block of the stored pivot rows in factored form (outer_u_form); [0]: offset +mp, [1]: -mp",
        "#define TF_UOUT_FACT 1",
        "// pattern of the outer block of A: [direction][equation][variable]",
        "static constexpr bool tf_uout_nz[2][%d][%d] = {%s};" % (
            nvar, nvar, ", ".join("{%s}" % ", ".join(bools(row) for row in nz) for nz in form["nz"])),
        "// S, the equations that reach the outer offset: the columns of Dinv that are stored",
        "static constexpr bool tf_uout_row[2][%d] = {%s};" % (nvar, ", ".join(bools(r) for r in form["rows"])),
        "// the value planes that feed the outer block",
        "static constexpr bool tf_uout_ld[2][%d] = {%s};" % (
            max(nnz, 1), ", ".join(bools([k in planes for k in range(max(nnz, 1))]) for planes in form["planes"])),
    ]


def lower_model(model, parvec_mask=0, seg=8, sweep_block=64):
    """Returns ``(source, spec)``: the per-model translation unit (without the
    skeleton includes' contents) and the dict of constants the runtime needs."""
    nvar = model._nvar
    fields = list(model._dep_vars) + list(model._help_funcs)
    nh = len(model._help_funcs)
    pars = list(model._pars)
    lo, hi = model._bounds
    mp = (model._window_range - 1) // 2
    if -lo != hi or hi != mp:
        raise UnsupportedExpression("asymmetric stencil window %r" % (model._bounds,))
    if mp < 1:
        mp = 1          # purely local models still get the width-3 skeleton
    if nvar + nh > 16 or len(pars) > 16:
        raise UnsupportedExpression("too many fields / parameters for the HIP skeleton")
    if mp * nvar > 16:
        # (the reduced levels of the banded solver are written for blocks of up to 16 x 16: 8 or 16 lanes
        # share a block row, tf_coop_hip.h; the reference takes any size, triflow/core/model.py:138-150)
        raise UnsupportedExpression(
            "the banded solver of the HIP back end handles b = (stencil half width) x (number of dependent "
            "variables) <= 16; this model has b = %d x %d = %d" % (mp, nvar, mp * nvar))
    sparse = [int(k) for k in model._sparse_indices[0]]
    nnz = len(sparse)
    real_mp = (model._window_range - 1) // 2
    pat_eq = [k % nvar for k in sparse]
    pat_var = [(k // nvar) % nvar for k in sparse]
    pat_off = [(k // nvar) // nvar - real_mp for k in sparse]

    mode = heaviside_mode(model)
    names, decls, uniform = _stencil_names(fields, pars, mp, parvec_mask)
    f_nodes = _printed_expressions(model._symbolic_args, model.F_array.tolist(), mode)
    j_nodes = _printed_expressions(model._symbolic_args, model._J_sparse_array.tolist(), mode)
    host_consts = {}

    def emit_all(nodes):
        first = _CEmitter(names, uniform, mode)     # pass 1: count divisor reuse
        for n in nodes:
            first.visit(n)
        second = _CEmitter(names, uniform, mode)
        second.shared = first.den_count
        second.host_consts = host_consts            # one table for F and J
        return second, [second.visit(n) for n in nodes]

    emit_f, f_c = emit_all(f_nodes)
    emit_j, j_c = emit_all(j_nodes)
    # (x may also sit only in a hoisted divisor: tf_denK = xc)
    uses_x = any("xc" in _tokens(s) for s in f_c + j_c + list(emit_f.denominators) + list(emit_j.denominators))

    # Jacobian entries that are the same at every node of a system (constant coefficients:
    # only dx, scalar parameters and constants): the solver kernels evaluate them once per
    # thread instead of reading them back from the value table at every node
    j_uniform = [1 if emit_j.is_uniform(n) else 0 for n in j_nodes]

    j_alias, j_alias_scale = _proportional_entries(model, j_uniform, mode)

    def body(outname, exprs, emitter, only=None):
        lines = ["    " + d for d in decls if only is None or d.split("=")[1].strip().startswith("par[")]
        lines += ["    const double* tf_hc = par + %d;" % len(pars)]
        lines += ["    (void)dx; (void)xc; (void)par; (void)tf_hc;"]
        # node-independent divisors and their reciprocals: loop invariant, hoisted
        # (uniform entries divide uniform numerators: plain division, no hoisted divisor)
        for den, k in sorted(emitter.denominators.items(), key=lambda kv: kv[1]) if only is None else ():
            lines += ["    const double tf_den%d = %s;" % (k, den),
                      "    const double tf_rden%d = 1.0 / tf_den%d;" % (k, k)]
        lines += ["    %s[%d] = %s;" % (outname, i, e) for i, e in enumerate(exprs)
                  if only is None or only[i]]
        return "\n".join(lines)

    def arr(name, values, ctype="int"):
        vals = ", ".join(str(v) for v in values) if values else "0"
        return "static constexpr %s %s[%d] = {%s};" % (ctype, name, max(len(values), 1), vals)

    blk_nz = block_mask(nvar, pat_eq, pat_var)
    blk_full = all(all(row) for row in blk_nz)
    u_outer = outer_u_form(nvar, mp, pat_eq, pat_var, pat_off, j_uniform, j_alias, blk_nz)
    hc_list = [src_ for src_, _ in sorted(host_consts.items(), key=lambda kv: kv[1])]
    par_is_vec = [1 if (parvec_mask >> k) & 1 else 0 for k in range(len(pars))] + [0] * len(hc_list)
    if len(pars) + len(hc_list) > 16:
        raise UnsupportedExpression("too many parameters + host constants for the HIP skeleton")
    src = "\n".join([
        "// generated by triflow_amd.codegen -- do not edit",
        "// equations: " + " ; ".join(str(e) for e in model._diff_eqs),
        *(["// heaviside: exact (Heaviside = numpy.heaviside, DiracDelta = 0, Piecewise = numpy.select)"]
          if mode == "exact" else []),
        "#define TF_NVAR %d" % nvar,
        "#define TF_NH %d" % nh,
        "#define TF_MP %d" % mp,
        "#define TF_NNZ %d" % nnz,
        "#define TF_NPAR %d" % (len(pars) + len(host_consts)),
        "#define TF_SEG %d" % seg,
        "#define TF_SWEEP_BLOCK %d" % sweep_block,
        "#define TF_USES_X %d" % (1 if uses_x else 0),
        arr("tf_pat_eq", pat_eq), arr("tf_pat_var", pat_var), arr("tf_pat_off", pat_off),
        "// entries of a solver block that can be non-zero (block_mask): [equation][variable]",
        "#define TF_BLK_FULL %d" % (1 if blk_full else 0),
        "static constexpr bool tf_blk_nz[%d][%d] = {%s};" % (
            nvar, nvar, ", ".join("{%s}" % ", ".join("true" if v else "false" for v in row) for row in blk_nz)),
        arr("tf_par_is_vec", par_is_vec, "bool"),
        arr("tf_j_uniform", j_uniform, "bool"),
        arr("tf_j_alias", j_alias), arr("tf_j_alias_scale", [_dbl(v) for v in j_alias_scale], "double"),
        *_outer_u_lines(u_outer, nvar, nnz),
        "TF_DEVICE void tf_eval_F(const double (&w)[TF_NVAR + TF_NH][2 * TF_MP + 1], "
        "const double* par, double dx, double xc, double* F) {",
        body("F", f_c, emit_f),
        "}",
        "TF_DEVICE void tf_eval_J(const double (&w)[TF_NVAR + TF_NH][2 * TF_MP + 1], "
        "const double* par, double dx, double xc, double* J) {",
        body("J", j_c, emit_j),
        "}",
        "// the node-independent entries only (tf_j_uniform); same expressions, same bits",
        "TF_DEVICE void tf_eval_J_uniform(const double* par, double dx, double* J) {",
        "    const double xc = 0.0;",
        body("J", j_c, emit_j, only=j_uniform),
        "}",
        ""])
    spec = dict(nvar=nvar, nh=nh, npar=len(pars) + len(hc_list), npar_model=len(pars),
                host_consts=hc_list, mp=mp, nnz=nnz, seg=seg,
                sweep_block=sweep_block, uses_x=int(uses_x), parvec_mask=int(parvec_mask),
                b2=mp * nvar, pat_eq=pat_eq, pat_var=pat_var, pat_off=pat_off, j_uniform=j_uniform,
                j_alias=j_alias, j_alias_scale=j_alias_scale,
                blk_nz=blk_nz, u_outer=u_outer, fields=fields, pars=pars, heaviside=mode)
    return src, spec


#: reductions of a device probe, in the order of the TF_PROBE_* kinds of csrc/tf_probe.h
PROBE_REDUCTIONS = ("sum", "mean", "integral", "max", "min", "argmax", "argmin")


def _lower_node_expressions(model, exprs, parvec_mask, extra_names=None, extra_uniform=(), extra_args=()):
    """What the probes and the recorders share: discretised SymPy expressions over the model's symbolic
    arguments, printed by the same lambdify call as F and emitted by the same ``_CEmitter``.  Returns
    the lines that open the per-node body (the window / parameter names, the hoisted divisors), the C
    expressions, the uniform powers / libm calls evaluated on the host, whether ``x`` is read, the
    model's parameter names and its mode of Heaviside / DiracDelta / Piecewise.  ``extra_names``: further
    printed names and their C expressions (``extra_uniform``: those that are the same at every node;
    ``extra_args``: their symbols, which follow the model's own in the lambdify call) -- the hooks' ``t``
    and ``at()`` reads."""
    fields = list(model._dep_vars) + list(model._help_funcs)
    pars = list(model._pars)
    mp = max((model._window_range - 1) // 2, 1)
    names, decls, uniform = _stencil_names(fields, pars, mp, parvec_mask)
    names.update(extra_names or {})
    uniform |= set(extra_uniform)
    import sympy
    mode = heaviside_mode(model)
    for e in exprs:
        # In the default mode Heaviside is identically one in F and J (the reference's module dictionary:
        # it only ever stands there as the derivative of Max / Min).  An observer is not differentiated: a
        # Heaviside in it is the user's own, and a step function that is one everywhere is not what they
        # wrote.  (In the exact mode it is what they wrote.)
        if mode == "one" and sympy.sympify(e).has(sympy.Heaviside):
            raise UnsupportedExpression("function 'Heaviside' is not supported in a probe or recorder: the HIP "
                                        "compiler takes it as identically one, as the reference does in J; "
                                        "write the step with Max / Min / sign" + _EXACT_HINT)
    nodes = _printed_expressions([*model._symbolic_args, *extra_args], list(exprs), mode)
    first = _CEmitter(names, uniform, mode)         # pass 1: count divisor reuse
    for n in nodes:
        first.visit(n)
    emit = _CEmitter(names, uniform, mode)
    emit.shared = first.den_count
    out = [emit.visit(n) for n in nodes]
    hc_list = [src_ for src_, _ in sorted(emit.host_consts.items(), key=lambda kv: kv[1])]
    uses_x = any("xc" in _tokens(c) for c in out + list(emit.denominators))
    lines = ["    " + d for d in decls]
    lines += ["    (void)dx; (void)xc; (void)par; (void)tf_hc;"]
    for den, k in sorted(emit.denominators.items(), key=lambda kv: kv[1]):
        lines += ["    const double tf_den%d = %s;" % (k, den),
                  "    const double tf_rden%d = 1.0 / tf_den%d;" % (k, k)]
    return lines, out, hc_list, uses_x, pars, mode


def lower_probes(model, exprs, reductions, parvec_mask=0):
    """Device probes -> ``(block, spec)``: the C block that follows the model's own translation unit
    (``TF_NPROBE`` ... and ``tf_eval_probe``, read by csrc/tf_probe.h) and the constants the runtime
    needs.  ``exprs`` are discretised SymPy expressions over the model's symbolic arguments
    (``probes.discretise``); they are printed by the same lambdify call as F and emitted by the same
    ``_CEmitter``, so the per-node values are the bits NumPy computes from the printed expressions.
    Uniform powers / libm calls become host constants of the probes (``spec["host_consts"]``, the
    probe's own argument buffer: the model's parameter slots are not touched)."""
    kinds = [PROBE_REDUCTIONS.index(r) for r in reductions]
    lines, out, hc_list, uses_x, pars, mode = _lower_node_expressions(model, exprs, parvec_mask)
    lines += ["    P[%d] = %s;" % (i, c) for i, c in enumerate(out)]
    block = "\n".join([
        "// device probes, generated by triflow_amd.codegen.lower_probes -- do not edit",
        "// " + " ; ".join("%s: %s" % (r, e) for r, e in zip(reductions, exprs)),
        "#define TF_NPROBE %d" % len(out),
        "#define TF_NPROBE_HC %d" % len(hc_list),
        "#define TF_PROBE_USES_X %d" % (1 if uses_x else 0),
        "static constexpr int tf_probe_kind[%d] = {%s};" % (max(len(kinds), 1),
                                                           ", ".join(map(str, kinds)) or "0"),
        "TF_DEVICE void tf_eval_probe(const double (&w)[TF_NVAR + TF_NH][2 * TF_MP + 1], "
        "const double* par, const double* tf_hc, double dx, double xc, double* P) {",
        "\n".join(lines),
        "}",
        ""])
    spec = dict(nprobe=len(out), kinds=kinds, host_consts=hc_list, pars=pars, uses_x=int(uses_x),
                heaviside=mode)
    return block, spec


#: pools of a device recorder, in the order of the TF_REC_* pools of csrc/tf_args.h
RECORD_POOLS = ("sample", "max", "min", "mean")


def _lower_switch(model, exprs, parvec_mask, stem, eval_name, count_key, words, wrapper):
    """The ``switch (k)`` block of the observers that evaluate one expression per call -> ``(block,
    spec)``: ``TF_N<stem>``, ``TF_N<stem>_HC``, ``TF_<stem>_USES_X`` (one stem serves the counts and the
    uses-x macro of every kind) and ``<eval_name>``, expression ``k`` being case ``k``;
    ``spec[count_key]`` counts the expressions.  ``words`` and ``wrapper``: the kind and the public
    function the header comment names."""
    lines, out, hc_list, uses_x, pars, mode = _lower_node_expressions(model, exprs, parvec_mask)
    lines += ["    switch (k) {"]
    lines += ["    case %d: return %s;" % (i, c) for i, c in enumerate(out)]
    lines += ["    default: return 0.0;", "    }"]
    block = "\n".join([
        "// %s, generated by triflow_amd.codegen.%s -- do not edit" % (words, wrapper),
        "// " + " ; ".join(str(e) for e in exprs),
        "#define TF_N%s %d" % (stem, len(out)),
        "#define TF_N%s_HC %d" % (stem, len(hc_list)),
        "#define TF_%s_USES_X %d" % (stem, 1 if uses_x else 0),
        "TF_DEVICE double %s(int k, const double (&w)[TF_NVAR + TF_NH][2 * TF_MP + 1], "
        "const double* par, const double* tf_hc, double dx, double xc) {" % eval_name,
        "\n".join(lines),
        "}",
        ""])
    spec = {count_key: len(out), "host_consts": hc_list, "pars": pars, "uses_x": int(uses_x), "heaviside": mode}
    return block, spec


def lower_records(model, exprs, parvec_mask=0):
    """Device recorders -> ``(block, spec)``: the C block that follows the model's own translation unit
    (``TF_NREC`` ... and ``tf_eval_record``, read by csrc/tf_record.h; expression ``k`` is case ``k``)
    and the constants the runtime needs.  Lowered as the probes are (``_lower_node_expressions``): the
    per-node values are the bits NumPy computes from the printed expressions; the host constants go
    into the recorders' own argument buffer (``spec["host_consts"]``)."""
    return _lower_switch(model, exprs, parvec_mask, "REC", "tf_eval_record", "nrec", "device recorders", "lower_records")


def lower_statistics(model, exprs, parvec_mask=0):
    """Device statistics -> ``(block, spec)``: the C block that follows the model's own translation unit
    (``TF_NSTAT`` ... and ``tf_eval_stat``, read by csrc/tf_stat.h; expression ``k`` is case ``k``) and
    the constants the runtime needs.  Lowered as the probes and the recorders are
    (``_lower_node_expressions``): the per-node values are the bits NumPy computes from the printed
    expressions; the host constants go into the statistics' own argument buffer (``spec["host_consts"]``)."""
    return _lower_switch(model, exprs, parvec_mask, "STAT", "tf_eval_stat", "nstat", "device statistics", "lower_statistics")


def lower_spectra(model, exprs, parvec_mask=0):
    """Device spectra -> ``(block, spec)``: the C block that follows the model's own translation unit
    (``TF_NSPEC`` ... and ``tf_eval_spectrum``, read by csrc/tf_spectrum.h; expression ``k`` is case ``k``)
    and the constants the runtime needs.  Lowered as the other observers are (``_lower_node_expressions``):
    the per-node values are the bits NumPy computes from the printed expressions; the host constants go
    into the spectra's own argument buffer (``spec["host_consts"]``).  The modes are not part of the
    block: spectra of the same expressions share a code object whatever their modes."""
    return _lower_switch(model, exprs, parvec_mask, "SPEC", "tf_eval_spectrum", "nspec", "device spectra", "lower_spectra")


def lower_extrema(model, exprs, parvec_mask=0):
    """Device extrema -> ``(block, spec)``: the C block that follows the model's own translation unit
    (``TF_NEXT`` ... and ``tf_eval_extrema``, read by csrc/tf_extrema.h; expression ``k`` is case ``k``)
    and the constants the runtime needs.  Lowered as the other observers are (``_lower_node_expressions``):
    the per-node values are the bits NumPy computes from the printed expressions; the host constants go
    into the extrema's own argument buffer (``spec["host_consts"]``).  Kind, threshold, ``max_count`` and
    ``every`` are not part of the block: they are launch arguments, and sets that differ only in them
    share a code object."""
    return _lower_switch(model, exprs, parvec_mask, "EXT", "tf_eval_extrema", "next", "device extrema", "lower_extrema")


def lower_histograms(model, exprs, parvec_mask=0):
    """Device histograms -> ``(block, spec)``: the C block that follows the model's own translation unit
    (``TF_NHIST`` ... and ``tf_eval_hist``, read by csrc/tf_histogram.h; expression ``k`` is case ``k``)
    and the constants the runtime needs.  Lowered as the other observers are (``_lower_node_expressions``):
    the per-node values are the bits NumPy computes from the printed expressions; the host constants go
    into the histograms' own argument buffer (``spec["host_consts"]``).  Edges, window and ``every`` are
    not part of the block: they are data of the handle and launch arguments, and sets that differ only in
    them share a code object.  ``TF_NHIST`` is also what makes csrc/tf_histogram.h emit its kernels: no
    other code object holds them."""
    return _lower_switch(model, exprs, parvec_mask, "HIST", "tf_eval_hist", "nhist", "device histograms", "lower_histograms")


#: kinds of a hook statement, in the order of TF_HOOK_POINT / TF_HOOK_WINDOW of csrc/tf_args.h
HOOK_KINDS = ("point", "window")


class HookStatement:
    """One statement ``fields[var][target] = expr`` of a hook program, laid out for a grid: ``kind`` of
    ``HOOK_KINDS``; ``var`` the index of the dependent variable; ``target`` the node ``0 ... N - 1`` (point)
    or ``(start, stop, step)`` = ``slice.indices(N)`` (window); ``expr`` a SymPy expression over the centre
    symbols of the model's fields, its parameters, ``x``, ``dx``, ``t`` and the symbols of ``at``;
    ``at``: ``(symbol, field index, node 0 ... N - 1)`` per ``at()`` read (point statements only)."""

    def __init__(self, kind, var, target, expr, at=()):
        self.kind, self.var, self.target, self.expr, self.at = kind, int(var), target, expr, tuple(at)

    @property
    def geometry(self):
        """``(kind, var, a, b, c)``: a point's node, 0, 0; a window's start, stop, step."""
        a, b, c = (self.target, 0, 0) if self.kind == "point" else self.target
        return (HOOK_KINDS.index(self.kind), self.var, int(a), int(b), int(c))


def hook_runs(statements):
    """``[(first, count)]``: the maximal runs of consecutive statements of one kind -- a launch each."""
    runs = []
    for k, st in enumerate(statements):
        if runs and statements[runs[-1][0]].kind == st.kind:
            runs[-1][1] += 1
        else:
            runs.append([k, 1])
    return [tuple(r) for r in runs]


def lower_hooks(model, statements, parvec_mask=0):
    """A hook program (``hooks.ExpressionHook``: :class:`HookStatement` in execution order) -> ``(block,
    spec)``: the C block that follows the model's own translation unit (``TF_NHOOK`` ... ``tf_eval_hook``,
    statement ``k`` being case ``k``, and the static tables of the statements: kind, target variable,
    target, ``at()`` reads as (field, node) pairs gathered per statement -- read by csrc/tf_hook.h) and the
    constants the runtime needs.  Lowered as the observers are (``_lower_node_expressions``): a value is the
    bits NumPy computes from the printed expression.  ``t`` is one more uniform name: a power or libm call
    of uniform arguments that reads it is a host constant, evaluated per call (``eval_host_constants(...,
    t=t)``), and a bare ``t`` is the host constant ``"t"`` itself, so nothing of ``t`` is a launch argument.
    ``spec["geometry"]`` is what ``tf_hook_create`` takes, ``spec["runs"]`` the launches of one application."""
    import sympy
    statements = list(statements)
    if not statements:
        raise ValueError("a hook program has one statement at least")
    maxat = max([len(st.at) for st in statements] + [1])
    at_syms = [sympy.Symbol("tf_at_%d" % j) for j in range(maxat)]
    exprs = []
    for st in statements:
        if st.kind not in HOOK_KINDS:
            raise ValueError("hook statement of unknown kind %r" % (st.kind,))
        if st.kind == "window" and st.at:
            raise UnsupportedExpression("at() in a window statement")
        exprs.append(sympy.sympify(st.expr).xreplace({sym: at_syms[j] for j, (sym, _, _) in enumerate(st.at)}))
    extra = {"t": "tf_t", **{"tf_at_%d" % j: "tf_at[%d]" % j for j in range(maxat)}}
    lines, out, hc_list, uses_x, pars, mode = _lower_node_expressions(
        model, exprs, parvec_mask, extra_names=extra, extra_uniform=("t",),
        extra_args=[sympy.Symbol("t"), *at_syms])
    if any("tf_t" in _tokens(text) for text in out + lines):
        # (a bare t: the last host constant, so it comes with the others and from the same buffer)
        hc_list = hc_list + ["t"]
        lines.insert(0, "    const double tf_t = tf_hc[%d];" % (len(hc_list) - 1))
    lines += ["    (void)tf_at;", "    switch (k) {"]
    lines += ["    case %d: return %s;" % (i, c) for i, c in enumerate(out)]
    lines += ["    default: return 0.0;", "    }"]
    geometry = [st.geometry for st in statements]
    at_first, at_field, at_node = [], [], []
    for st in statements:
        at_first.append(len(at_field))
        at_field += [int(f) for _, f, _ in st.at]
        at_node += [int(g) for _, _, g in st.at]

    def arr(name, values):
        return "static constexpr int %s[%d] = {%s};" % (name, max(len(values), 1),
                                                        ", ".join(str(int(v)) for v in values) or "0")
    n = len(statements)
    block = "\n".join([
        "// device hooks, generated by triflow_amd.codegen.lower_hooks -- do not edit",
        *("// %s %d: %s[%s] = %s" % (st.kind, k, st.var, st.target, e)
          for k, (st, e) in enumerate(zip(statements, exprs))),
        "#define TF_NHOOK %d" % n,
        "#define TF_NHOOK_HC %d" % len(hc_list),
        "#define TF_HOOK_USES_X %d" % (1 if uses_x else 0),
        "#define TF_HOOK_MAXAT %d" % maxat,
        "// per statement: kind (0 point, 1 window), target variable, target (node, 0, 0 / start, stop, step)",
        arr("tf_hook_kind", [g[0] for g in geometry]), arr("tf_hook_var", [g[1] for g in geometry]),
        arr("tf_hook_a", [g[2] for g in geometry]), arr("tf_hook_b", [g[3] for g in geometry]),
        arr("tf_hook_c", [g[4] for g in geometry]),
        "// the at() reads of a statement: tf_hook_nat of them from tf_hook_at0 on, (field, node) pairs",
        arr("tf_hook_nat", [len(st.at) for st in statements]), arr("tf_hook_at0", at_first),
        arr("tf_hook_at_field", at_field), arr("tf_hook_at_node", at_node),
        "TF_DEVICE double tf_eval_hook(int k, const double (&w)[TF_NVAR + TF_NH][2 * TF_MP + 1], "
        "const double* par, const double* tf_hc, double dx, double xc, const double* tf_at) {",
        "\n".join(lines),
        "}",
        ""])
    spec = dict(nhook=n, host_consts=hc_list, pars=pars, uses_x=int(uses_x), heaviside=mode,
                geometry=geometry, runs=hook_runs(statements), maxat=maxat)
    return block, spec


def _proportional_entries(model, j_uniform, heaviside="one"):
    """Jacobian entries that are an exact power-of-two multiple of an earlier node-dependent
    entry (``-q*dxT/h`` differentiated with respect to ``T_m1`` and ``T_p1``; ``We*h*dxxxh`` with
    respect to the four neighbours of ``h``; a reaction term that enters two equations with
    opposite signs): the kernels that read the value table back load one of them and scale.
    ``alias[k]`` = index of the entry to load (-1: none), ``scale[k]`` = +-2**n.  Accepted only if
    (i) SymPy proves the proportionality and (ii) the two expressions, evaluated the way the
    reference evaluates them (the lambdified NumPy code whose operation tree the C code repeats),
    agree *bit for bit* on random inputs -- scaling by a power of two commutes with every
    rounding, a different association of the same product would not.  In the exact mode an entry with a
    Heaviside, a DiracDelta or a Piecewise is never an alias and never the source of one: random samples
    do not visit its kinks."""
    exprs = model._J_sparse_array.tolist()
    nnz = len(exprs)
    alias, scale = [-1] * nnz, [1.0] * nnz
    cand = [k for k in range(nnz) if not j_uniform[k]]
    if heaviside == "exact":
        import sympy
        cand = [k for k in cand if not sympy.sympify(exprs[k]).has(sympy.Heaviside, sympy.DiracDelta,
                                                                   sympy.Piecewise)]
    if len(cand) < 2:
        return alias, scale
    func = lambdify(model._symbolic_args, exprs, modules=LAMBDIFY_MODULES[heaviside], cse=False)
    rng = np.random.default_rng(12345)
    samples = []
    for _ in range(2):
        args = [rng.uniform(0.5, 2.0, 257) * rng.choice([-1.0, 1.0], 257) for _ in model._symbolic_args]
        with np.errstate(all="ignore"):
            vals = func(*args)
        samples.append([np.broadcast_to(np.asarray(v, dtype=float), (257,)) for v in vals])
    for k in cand:
        for m in cand:
            if m >= k:
                break
            if alias[m] >= 0:
                continue
            a0, b0 = samples[0][k], samples[0][m]
            if not (np.isfinite(a0).all() and np.isfinite(b0).all()) or not np.all(b0 != 0.0):
                continue
            r = a0[0] / b0[0]
            mant, _ = np.frexp(abs(r))
            if not (np.isfinite(r) and r != 0.0 and mant == 0.5):
                continue
            if not all(np.array_equal(smp[k], r * smp[m]) for smp in samples):
                continue
            if sympy_simplify(exprs[k] - sympy_Float_exact(r) * exprs[m]) != 0:
                continue
            alias[k], scale[k] = m, float(r)
            break
    return alias, scale


def sympy_Float_exact(r):
    import sympy
    return sympy.Rational(*float(r).as_integer_ratio())


def sympy_simplify(e):
    import sympy
    return sympy.simplify(e)


_HOST_NS = {name: getattr(np, name) for name in
            ("sqrt", "exp", "log", "sin", "cos", "tan", "tanh", "sinh", "cosh", "arctan", "arcsin",
             "arccos", "log10", "log2", "cbrt", "expm1", "log1p", "maximum", "minimum", "pi")}
_HOST_NS["E"] = _HOST_NS["e"] = np.e
# a uniform Heaviside / Piecewise inside a hoisted power or libm call: the meaning of its mode
_HOST_NS_MODE = {
    "one": {"Heaviside": lambda *a: np.float64(1.0)},
    "exact": {"Heaviside": np.heaviside, "DiracDelta": _dirac_zero, "select": np.select, "nan": np.nan,
              **{name: getattr(np, name) for name in (*_COMPARE, "logical_and", "logical_or", "logical_not")}},
}


def eval_host_constants(spec, dx, par_values, t=None):
    """Values of the model's uniform power / libm sub-expressions for one system,
    computed exactly as the reference's lambdified NumPy code computes them.  ``t``: the time a hook is
    called with (the host constants of a hook program may read it)."""
    env = {name: np.float64(np.ravel(v)[0]) for name, v in zip(spec["pars"], par_values)}
    env["dx"] = np.float64(dx)
    if t is not None:
        env["t"] = np.float64(t)
    out = []
    for src_ in spec["host_consts"]:
        with np.errstate(all="ignore"):
            out.append(float(eval(src_, {"__builtins__": {}, **_HOST_NS,
                                         **_HOST_NS_MODE[spec.get("heaviside", "one")]}, env)))
    return out


def _tokens(text):
    out, cur = set(), ""
    for ch in text:
        if ch.isalnum() or ch == "_":
            cur += ch
        else:
            if cur:
                out.add(cur)
            cur = ""
    if cur:
        out.add(cur)
    return out


def source_hash(*parts):
    h = hashlib.sha256()
    for part in parts:
        h.update(part if isinstance(part, bytes) else str(part).encode())
        h.update(b"\0")
    return h.hexdigest()[:20]
