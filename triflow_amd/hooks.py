"""Expression hooks: boundary and whole-field hooks written in the model's own string language.

A hook is the reference's only mechanism for boundary conditions and for anything else done to the state
between steps: ``hook(t, fields, pars) -> fields, pars``, called at ``t`` on the input of every step and at
``t + dt`` on its result.  An :class:`ExpressionHook` is a program of statements::

    hook = ExpressionHook(model, [
        ("h", 0,                 "1 + A * sin(2 * pi * f * t)"),   # point statement: a forced inlet
        ("q", 0,                 "h * h * h / 3"),                 # sees the h[0] just written
        ("h", -1,                "at(h, -2)"),                     # outflow: copy of another node
        ("q", -1,                "2 * at(q, -2) - at(q, -3)"),     # linear extrapolation
        ("h", slice(-400, None), "h - s * (h - 1)"),               # window statement: a sponge
        ("h", slice(None),       "Max(h, 1e-6)"),                  # whole-field clip
    ])

whose contract is the Python function that executes them **in the order given**: each statement is
``fields[var][target] = value`` with the right-hand side evaluated completely before the assignment
(NumPy's rule), and each statement sees the assignments of the statements before it.  ``__call__`` is that
function, on host arrays, from the lambdified expressions -- so the object is a valid hook for the
reference's own ``Simulation`` and for host containers -- and the device schemes of this package run the
same program with two kernels on the state where it lives (``csrc/tf_hook.h``, ``codegen.lower_hooks``),
at the places and with the times the reference calls ``hook``.

Names in an expression: the model's dependent variables and help functions are the value at the target
node (point) or at the node being assigned (window); the model's parameters (per-node arrays included);
``x`` the coordinate of that node; ``t`` the time the hook is called with; constants and the function
vocabulary of the model language.  In a point statement only, ``at(name, k)`` is field ``name`` at the
absolute node ``k`` (an integer literal, negative values counted from the end).  An expression is evaluated
as SymPy prints it after parsing (not expanded): ``h * h * h`` is ``h**3``.

Refused with ``ValueError`` naming the statement: derivatives and ``upwind(...)`` (anything that
discretises to an off-centre node), ``at()`` in a window statement (the kernel assigns in place: both
would read what another thread is writing), ``Heaviside`` on a model in the default mode (as in every
observer), unknown symbols.
"""

import re

import numpy as np
import sympy as sp
from sympy.core.function import AppliedUndef

from . import codegen

__all__ = ["ExpressionHook"]


def _is_int(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))


class _Statement:
    """One parsed statement: ``var`` (name), ``target`` (int or slice), ``expression`` (the string), ``expr``
    (SymPy, over the centre symbols), ``at`` ((symbol, field name, node as written) per ``at()`` read)."""

    def __init__(self, index, var, target, expression, expr, at, args, mode):
        self.index, self.var, self.target, self.expression = index, var, target, expression
        self.expr, self.at = expr, at
        self.kind = "point" if _is_int(target) else "window"
        self._args, self._mode, self._fn = args, mode, None

    def label(self):
        return "statement %d (%s[%r] = %r)" % (self.index, self.var, self.target, self.expression)

    @property
    def function(self):
        """The lambdified right-hand side: ``f(x, *fields, *pars, dx, t, *at)`` (the printer, and so the
        operation tree, of the device code)."""
        if self._fn is None:
            self._fn = sp.lambdify([*self._args, *(s for s, _, _ in self.at)], self.expr,
                                   modules=codegen.LAMBDIFY_MODULES[self._mode], cse=False)
        return self._fn


class ExpressionHook:
    """``ExpressionHook(model, statements, parameters=None)``: see the module's docstring.  ``statements``:
    ``(var, target, expression)`` with ``var`` a dependent variable, ``target`` an integer node (point
    statement; negative: from the end; checked against the grid at first use) or a slice with a step >= 1
    (window statement; an empty window is legal and does nothing).  ``parameters``: a callable ``(t, pars)
    -> dict`` of parameter updates, as in :class:`~triflow_amd.device.DirichletHook` (host side).

    On the device a program costs one launch per maximal run of consecutive statements of one kind (the
    example of the module's docstring: 2).  ``idempotent`` is derived: true iff no right-hand side reads a
    field (only ``t``, ``x``, parameters and constants); such a program may be skipped on an input that holds
    its values already, any other one is applied every time the reference would call it.
    ``schemes.BDF2`` takes the device path only for an idempotent program (its step hooks its input in
    place) and uses any other one as the callable it is."""

    def __init__(self, model, statements, parameters=None):
        self.model = model
        self.parameters = parameters
        statements = list(statements)
        if not statements:
            raise ValueError("an ExpressionHook has one statement at least")
        self._fields = list(model._dep_vars) + list(model._help_funcs)
        self._pars = list(model._pars)
        self._mode = codegen.heaviside_mode(model)
        self._args = [sp.Symbol("x"), *map(sp.Symbol, self._fields), *map(sp.Symbol, self._pars),
                      sp.Symbol("dx"), sp.Symbol("t")]
        self.statements = [self._parse(k, st) for k, st in enumerate(statements)]
        self._layouts = {}           # N -> [codegen.HookStatement]
        self._blocks = {}            # (N, parvec mask) -> (block, spec)

    # ---- parsing ---------------------------------------------------------------------------
    def _parse(self, index, statement):
        try:
            var, target, expression = statement
        except (TypeError, ValueError):
            raise ValueError("statement %d: %r, a triple (variable, target, expression) is expected"
                             % (index, statement))
        label = "statement %d (%s[%r] = %r)" % (index, var, target, expression)
        model = self.model
        if var not in model._dep_vars:
            raise ValueError("%s: %r is not a dependent variable of the model (%s)"
                             % (label, var, ", ".join(model._dep_vars)))
        if isinstance(target, slice):
            try:
                window = target.indices(1 << 30)
            except (TypeError, ValueError) as exc:
                raise ValueError("%s: %s" % (label, exc))
            if window[2] < 1:
                raise ValueError("%s: a window has a step >= 1" % label)
        elif not _is_int(target):
            raise ValueError("%s: the target is an integer node or a slice" % label)
        if not isinstance(expression, str):
            raise ValueError("%s: the right-hand side is a string of the model's language" % label)
        try:
            (expr,) = model._parse_strings((expression,))
        except ValueError:
            raise ValueError("%s: badly formated expression" % label)
        # at(name, k) -> a symbol of its own; the reads are gathered before the statement's value is formed
        at, repl = [], {}
        calls = sorted((c for c in expr.atoms(AppliedUndef) if c.func.__name__ == "at"), key=str)
        for call in calls:
            if isinstance(target, slice):
                raise ValueError("%s: at() in a window statement: the kernel assigns in place, and the read "
                                 "would see what another thread is writing (out of scope: it needs an "
                                 "out-of-place application)" % label)
            name = None
            if len(call.args) == 2:
                a0 = call.args[0]
                name = str(a0.func) if isinstance(a0, AppliedUndef) else (str(a0) if a0.is_Symbol else None)
            if name not in self._fields or not call.args[1].is_Integer:
                raise ValueError("%s: %s, at(name, k) takes a field of the model and an integer literal"
                                 % (label, call))
            sym = sp.Symbol("tf_at_%d" % len(at))
            repl[call] = sym
            at.append((sym, name, int(call.args[1])))
        expr = expr.xreplace(repl)
        # what discretises to an off-centre node is refused: looked for in the discretised expression's symbols
        if expr.has(sp.Derivative) or any(f.func.__name__ == "upwind" for f in expr.atoms(AppliedUndef)):
            off = True
        else:
            off = False
        work = object.__new__(type(model))
        work.__dict__.update(model.__dict__)
        work._symb_vars_with_spatial_diff_order = {k: set(v) for k, v in
                                                    model._symb_vars_with_spatial_diff_order.items()}
        try:
            (disc,) = work._discretise((expr,))
        except NotImplementedError as exc:
            raise ValueError("%s: %s" % (label, exc))
        allowed = set(self._args) | {s for s, _, _ in at}
        pattern = re.compile(r"^(%s)_[mp]\d+$" % "|".join(re.escape(f) for f in self._fields))
        stray = sorted(str(s) for s in sp.sympify(disc).free_symbols - allowed)
        if off or any(pattern.match(s) for s in stray):
            raise ValueError("%s: derivatives and upwind() are refused: a hook statement reads the node it "
                             "assigns (and, in a point statement, the nodes named with at()), and this one "
                             "discretises to %s" % (label, ", ".join(s for s in stray if pattern.match(s))
                                                    or "a neighbour"))
        to_symbol = {f: sp.Symbol(str(f.func)) for f in model._symb_dep_vars + model._symb_help_funcs}
        expr = sp.sympify(expr.xreplace(to_symbol))
        unknown = sorted(str(s) for s in expr.free_symbols - allowed)
        undefined = sorted(str(f.func) + "(...)" for f in expr.atoms(AppliedUndef))
        if unknown or undefined:
            raise ValueError("%s: unknown %s" % (label, ", ".join(unknown + undefined)))
        st = _Statement(index, var, target, expression, expr, at, self._args, self._mode)
        try:                                         # (what the C emitter refuses, refused now)
            codegen.lower_hooks(model, [self._lay_out(st, None)])
        except codegen.UnsupportedExpression as exc:
            raise ValueError("%s: %s" % (label, exc))
        return st

    # ---- properties ------------------------------------------------------------------------
    def _reads(self, st):
        return {str(s) for s in st.expr.free_symbols}

    @property
    def idempotent(self):
        """No right-hand side reads a field: applying the program twice is applying it once."""
        return not any(st.at or self._reads(st) & set(self._fields) for st in self.statements)

    @property
    def time_dependent(self):
        return any("t" in self._reads(st) for st in self.statements)

    def update_pars(self, t, pars):
        if self.parameters is None:
            return pars
        new = dict(pars)
        new.update(self.parameters(t, pars))
        return new

    # ---- the contract, on host arrays -------------------------------------------------------------
    def __call__(self, t, fields, pars):
        pars = self.update_pars(t, pars)
        x = np.asarray(fields["x"])
        N = x.size
        dx = (x[-1] - x[0]) / (N - 1)
        for st, laid in zip(self.statements, self.layout(N)):
            if st.kind == "point":
                at = laid.target
                atv = [fields[self._fields[f]][g] for _, f, g in laid.at]
            else:
                at = slice(*laid.target)
                atv = []
                if laid.target[1] <= laid.target[0]:
                    continue
            fv = [fields[name][at] for name in self._fields]
            pv = [pars[k] if np.ndim(pars[k]) == 0 or np.size(pars[k]) == 1 else np.asarray(pars[k])[at]
                  for k in self._pars]
            with np.errstate(all="ignore"):
                value = st.function(x[at], *fv, *pv, dx, t, *atv)
            if st.kind == "point":
                fields[st.var][at] = np.float64(value)
            else:
                fields[st.var][at] = value
        return fields, pars

    # ---- laid out for a grid -----------------------------------------------------------------
    def _lay_out(self, st, N):
        """``st`` as a ``codegen.HookStatement`` for ``N`` nodes (None: any grid, for the checks of ``_parse``)."""
        var = list(self.model._dep_vars).index(st.var)

        def node(g, what):
            if N is None:
                return 0
            if not -N <= g < N:
                raise ValueError("%s: %s %d is out of range for a grid of %d nodes" % (st.label(), what, g, N))
            return g % N
        at = [(sym, self._fields.index(name), node(g, "at(%s, ...): node" % name)) for sym, name, g in st.at]
        if st.kind == "point":
            return codegen.HookStatement("point", var, node(int(st.target), "node"), st.expr, at)
        return codegen.HookStatement("window", var, st.target.indices(N if N is not None else 1 << 30), st.expr)

    def layout(self, N):
        """The statements for a grid of ``N`` nodes; ``ValueError`` for a node out of range."""
        N = int(N)
        if N not in self._layouts:
            self._layouts[N] = [self._lay_out(st, N) for st in self.statements]
        return self._layouts[N]

    def lowered(self, N, parvec_mask=0):
        """``codegen.lower_hooks`` of the program for ``N`` nodes and a parameter layout: ``(block, spec)``."""
        key = (int(N), int(parvec_mask))
        if key not in self._blocks:
            self._blocks[key] = codegen.lower_hooks(self.model, self.layout(N), parvec_mask=parvec_mask)
        return self._blocks[key]

    def launches(self, N):
        """Kernel launches of one application on a grid of ``N`` nodes: the runs with something to assign."""
        laid = self.layout(N)
        return sum(1 for first, count in codegen.hook_runs(laid)
                   if laid[first].kind == "point" or any(s.target[1] > s.target[0] for s in laid[first:first + count]))
