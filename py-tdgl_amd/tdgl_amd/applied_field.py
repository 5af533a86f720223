"""A solver's applied vector potential A(t): one small class per kind, chosen once when the solver is built
(`from_parameter`, `from_dimensionless`).  A field issues its own library calls, so no other module asks which kind it
has.  All arrays are dimensionless, ``[m, 2]``, on the edge centres.

kind       A(t)                                         evaluated by
static     A                                            nobody
callable   func(t)                                      the host, uploaded before every step
scaled     factor(t) * base, any uniform factor         the host evaluates the factor, the base stays on the device
ramp       LinearRamp(**ramp)(t) * base                 the device (tdgl_set_link_ramp)
table      TabulatedRamp(*table)(t) * base              the device (tdgl_set_link_table)
terms      A0 + f_1(t) A_1 + ... + f_K(t) A_K           the device (tdgl_set_link_terms)
loops      (a static or a terms field) + moving loops   the device (tdgl_set_link_loops)
"""

import numpy as np

from .hipcore import link_loops_args
from .parameter import FIELD_TERMS_MAX, LinearRamp, TabulatedRamp, _loop_potential


class AppliedField:
    """The static kind and the base of the others.  ``initial``: the A the solver starts with.  For the ensemble's
    messages: ``refusal``, the tail of the sentence that refuses this kind in a replica (None: accepted), and ``noun``,
    what a kind the device evaluates is called."""

    kind = "static"
    time_dependent = on_device = False
    refusal = noun = None

    def __init__(self, A, initial=None):
        self.A = A
        self.initial = self.value(0) if initial is None else initial

    def value(self, t):
        """The host's evaluation of A(t)."""
        return self.A

    def install(self, operators):
        """Set this field on a single solver; a kind whose A only the device knows returns it."""
        operators.set_link_exponents(self.initial)

    def install_replica(self, ens, r, A_initial) -> None:
        """Set this field on replica ``r`` of an ensemble, which has refused a kind with a ``refusal`` before."""
        ens.set_link_exponents(r, A_initial)

    def advance(self, ctx, time, dt_prev):
        """The host's work before a step; returns the new A where the host evaluated it."""

    def applied(self, source):
        """The A of the last step taken, from a `TDGLContext` or an ensemble replica; None: the caller's copy holds."""


class CallableField(AppliedField):
    kind, time_dependent = "callable", True
    refusal = "this one is not of that form."

    def __init__(self, func, initial=None):
        self.value = func
        super().__init__(None, initial)

    def advance(self, ctx, time, dt_prev):
        A = np.asarray(self.value(time), dtype=float)
        ctx.update_link_exponents(A, dt_prev)
        return A


class ScaledField(AppliedField):
    """A(t) = factor(t) * base (the reference's field-ramp example): ``base`` stays on the device."""

    kind, time_dependent = "scaled", True
    refusal = "this one's time factor is not a LinearRamp or a TabulatedRamp."

    def __init__(self, base, factor, initial=None):
        self.base, self.factor = np.asarray(base, dtype=float), factor
        super().__init__(None, initial)

    def value(self, t):
        return self.factor(t) * self.base

    def install(self, operators):
        operators.ctx.set_link_exponents_base(self.base, self.factor(0))

    def advance(self, ctx, time, dt_prev):
        ctx.update_link_scale(self.factor(time), dt_prev)

    def applied(self, source):  # (the links may lag behind it)
        return source.link_scale() * self.base


class RampField(ScaledField):
    """``factor``: a `LinearRamp`, which tdgl_run evaluates itself."""

    kind, noun, on_device, refusal = "ramp", "a field ramp", True, None
    advance = AppliedField.advance

    def __init__(self, base, factor, initial=None):
        self.ramp = factor.ramp
        super().__init__(base, factor.scalar, initial)

    def install(self, operators):
        super().install(operators)
        operators.ctx.set_link_ramp(**self.ramp)

    def install_replica(self, ens, r, A_initial):
        ens.set_link_ramp(r, self.base, **self.ramp)


class TableField(ScaledField):
    """``factor``: a `TabulatedRamp`, which tdgl_run evaluates itself."""

    kind, noun, on_device, refusal = "table", "a field table", True, None
    advance = AppliedField.advance

    def __init__(self, base, factor, initial=None):
        self.table = (factor.table.times, factor.table.values)
        super().__init__(base, factor.scalar, initial)

    def install(self, operators):
        super().install(operators)
        operators.ctx.set_link_table(*self.table)

    def install_replica(self, ens, r, A_initial):
        ens.set_link_table(r, self.base, *self.table)


class TermsField(AppliedField):
    """``terms``: a list of ``(A_k[m, 2], spec_k)``, ``spec_k`` a ramp's ``dict(tmin, tmax, initial, final)`` or a
    table's ``(times, values)``; ``A0`` may be None."""

    kind, noun = "terms", "a sum of field terms"
    time_dependent = on_device = True

    def __init__(self, A0, terms, initial=None):
        terms = list(terms)
        if not 1 <= len(terms) <= FIELD_TERMS_MAX:
            raise ValueError(f"vector_potential_terms: between 1 and {FIELD_TERMS_MAX} terms, got {len(terms)}.")
        factors = [LinearRamp(**spec) if isinstance(spec, dict) else TabulatedRamp(*spec) for _, spec in terms]
        self.factors = [f.scalar for f in factors]
        self.A0 = None if A0 is None else np.asarray(A0, dtype=float)
        self.terms = [(np.asarray(base, dtype=float), _spec(f)) for (base, _), f in zip(terms, factors)]
        super().__init__(None, initial)

    def value(self, t):
        return self.terms_value([f(t) for f in self.factors])

    def terms_value(self, scales) -> np.ndarray:
        """``((A0 + s_1 A_1) + s_2 A_2) + ...`` left to right, every product rounded before it is added (NumPy does not
        contract): the device's value for the same factors, bit for bit."""
        A = scales[0] * self.terms[0][0]
        if self.A0 is not None:
            A = self.A0 + A
        for s, (base, _) in zip(scales[1:], self.terms[1:]):
            A = A + s * base
        return A

    def install(self, operators):
        operators.ctx.set_link_terms(self.A0, self.terms)

    def install_replica(self, ens, r, A_initial):
        ens.set_link_terms(r, self.A0, self.terms)

    def applied(self, source):  # from the factors the time loop evaluated
        return self.terms_value(source.link_term_scales())


class LoopsField(AppliedField):
    """Moving current loops on top of ``under``, a static or a terms field: ``loops`` a list of ``dict(times,
    centers[n, 3], currents[n], radius)`` in the units of ``edge_centres``, currents dimensionless."""

    kind, time_dependent, on_device = "loops", True, True
    refusal = "a MovingCurrentLoop is evaluated on the device by solve() alone, not per replica."

    def __init__(self, under, loops, edge_centres, z_film, initial=None):
        self.under, self.loops, self.z_film = under, list(loops), float(z_film)
        self.edge_centres = np.asarray(edge_centres, dtype=float)
        link_loops_args(len(self.edge_centres), self.edge_centres, z_film, loops)  # (its refusals, before any device work)
        self.terms_value = getattr(under, "terms_value", None)
        super().__init__(None, initial)

    def value(self, t):
        ex, ey = self.edge_centres[:, 0], self.edge_centres[:, 1]
        A = self.under.value(t)
        for lp in self.loops:
            c = [float(np.interp(t, lp["times"], lp["centers"][:, j])) for j in range(3)]
            A = A + _loop_potential(ex, ey, self.z_film, c, lp["radius"], float(np.interp(t, lp["times"], lp["currents"])))[:, :2]
        return A

    def install(self, operators):
        self.under.install(operators)
        operators.ctx.set_link_loops(self.edge_centres, self.z_film, self.loops)
        return operators.ctx.link_exponents()  # the device's own A: what is saved is what was applied

    def applied(self, source):
        return source.link_exponents()


def _spec(factor):
    return factor.ramp if factor.ramp is not None else (factor.table.times, factor.table.values)


def from_parameter(applied, edge_centres, z0, A_scale, z_film) -> AppliedField:
    """The field of ``applied_vector_potential`` -- a `Parameter`, another callable or a uniform field's number, in the
    solver's units -- on the edge centres (solver.py:158-189, 347-362), scaled by ``A_scale`` to dimensionless units."""
    from .solver import uniform_field_vector_potential

    ex, ey = edge_centres[:, 0], edge_centres[:, 1]
    on_edges = lambda q, **kw: A_scale * np.asarray(q(ex, ey, z0, **kw))[:, :2]  # noqa: E731
    summed = lambda static, products: TermsField(  # noqa: E731
        None if static is None else on_edges(static), [(on_edges(q), _spec(f)) for f, q in products])
    if not getattr(applied, "time_dependent", False):
        return AppliedField(on_edges(applied) if callable(applied) else
                            A_scale * uniform_field_vector_potential(ex, ey, float(applied))[:, :2])
    sep = applied.separable_product() if hasattr(applied, "separable_product") else None
    if sep is not None:
        # a single product with no static part keeps its own path, call for call: the factor is evaluated per step, by
        # tdgl_run itself for a LinearRamp or a TabulatedRamp
        factor, static = sep
        if factor.ramp is not None:
            return RampField(on_edges(static), factor)
        if getattr(factor, "table", None) is not None:
            return TableField(on_edges(static), factor)
        return ScaledField(on_edges(static), factor.scalar)
    # anything else that is a sum of a static field and such products goes to the device as terms ...
    terms = applied.separable_terms() if hasattr(applied, "separable_terms") else None
    if terms is not None and terms[1]:
        return summed(*terms)
    # ... and with MovingCurrentLoop leaves in the sum, the loops ride on top of the terms or of the static part
    sources = applied.device_sources() if terms is None and hasattr(applied, "device_sources") else None
    if sources is not None and sources[2]:
        static, products, loops = sources
        under = summed(static, products) if products else AppliedField(
            np.zeros_like(edge_centres) if static is None else on_edges(static))
        return LoopsField(under, [dict(times=lp["times"], centers=lp["centers"], radius=lp["radius"],
                                       currents=A_scale * lp["unit_factor"] * lp["currents"]) for lp in loops],
                          edge_centres, z_film)
    return CallableField(lambda t: on_edges(applied, t=t))  # solver.py:347-362


def from_dimensionless(edge_centres, link_exponents=None, vector_potential_func=None, ramp=None, table=None, terms=None,
                       loops=None) -> AppliedField:
    """The field of `TDGLSolver.from_dimensionless`'s keyword arguments.  ``link_exponents``: the A the solver starts
    with (under loops without terms: their static part too); None: the field's value at t = 0."""
    A = None if link_exponents is None else np.asarray(link_exponents, dtype=float)
    if ramp is not None and table is not None:
        raise ValueError("vector_potential_ramp and vector_potential_table exclude each other.")
    for name, given in (("vector_potential_terms", terms is not None), ("vector_potential_loops", bool(loops))):
        if given and (ramp is not None or table is not None):
            raise ValueError(f"{name} excludes vector_potential_ramp and vector_potential_table.")
    if loops:
        full = []
        for lp in loops:
            c = np.asarray(lp["centers"], dtype=float)
            if c.ndim == 2 and c.shape[1] == 2:
                c = np.column_stack([c, float(lp["z"]) * np.ones(len(c))])
            full.append(dict(times=np.asarray(lp["times"], dtype=float), centers=c, radius=float(lp["radius"]),
                             currents=np.asarray(lp["currents"], dtype=float) * np.ones(len(c))))
        under = TermsField(*terms) if terms is not None else AppliedField(np.zeros((len(edge_centres), 2)) if A is None else A)
        return LoopsField(under, full, edge_centres, 0.0, A)
    if terms is not None:
        return TermsField(*terms, initial=A)
    if ramp is not None:
        return RampField(ramp[0], LinearRamp(**ramp[1]), A)
    if table is not None:
        return TableField(table[0], TabulatedRamp(*table[1:]), A)
    return AppliedField(A) if vector_potential_func is None else CallableField(vector_potential_func, A)
