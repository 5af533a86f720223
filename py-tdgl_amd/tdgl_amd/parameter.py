"""``Parameter``: a function of position (and optionally time) with keyword arguments bound, with
the behaviour of the reference's (`tdgl/parameter.py:66-439`): ``func(x, y[, z], **kwargs)`` checked
at construction, ``time_dependent=True`` for functions with a keyword-only ``t``, calls with or
without ``z`` / ``t``, ``+ - * / **`` between parameters and numbers giving ``CompositeParameter``,
equality by code and arguments, pickling, readable ``repr``.  The reference's result cache is not
kept (here a static parameter is evaluated once and lives on the device).  Additions used by the
solver: a factor that does not depend on position is recognised (``uniform_in_space``), so that
``A(t) = f(t) * A_static(r)`` keeps ``A_static`` on the device (``separable_product``).
"""

import inspect
import operator
from numbers import Number
from typing import Callable, Optional, Union

import numpy as np


def function_repr(func: Callable, argspec=None) -> str:
    """``name(arg, kw=default, *, kwonly=default)`` of a function (`tdgl/parameter.py:31-63`);
    ``argspec`` may be any object with the attributes of ``inspect.FullArgSpec``."""
    if argspec is None:
        argspec = inspect.getfullargspec(func)
    get = lambda name: getattr(argspec, name, None)  # noqa: E731
    args = [str(a) for a in (get("args") or [])]
    for k, val in enumerate(list(get("defaults") or [])[::-1]):
        args[-(k + 1)] += f"={val!r}"
    if get("varargs"):
        args.append("*" + get("varargs"))
    if get("kwonlyargs"):
        if not get("varargs"):
            args.append("*")
        args.extend(get("kwonlyargs"))
    for k, name in enumerate(args):
        if get("kwonlydefaults") and name in get("kwonlydefaults"):
            args[k] += f"={get('kwonlydefaults')[name]!r}"
    if get("varkw"):
        args.append("**" + get("varkw"))
    for k, name in enumerate(args):
        if get("annotations") and name in get("annotations"):
            args[k] += f": {getattr(get('annotations')[name], '__name__', get('annotations')[name])!r}"
    return getattr(func, "__name__", "func") + "(" + ", ".join(args) + ")"


class _BoundArgs:
    """argspec stand-in listing a parameter's bound keyword arguments (for ``repr``)."""

    def __init__(self, names, values):
        self.args, self.defaults = list(names), list(values)


def _same(a, b) -> bool:
    if a is b:
        return True
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return a.shape == b.shape and bool(np.allclose(a, b))
    try:
        return bool(a == b)
    except (TypeError, ValueError):
        return False


class Parameter:
    """``Parameter(func, time_dependent=False, **kwargs)``.

    ``func`` takes ``x, y`` (and optionally ``z`` as third argument) positionally; everything else
    must be a keyword argument (with a default, or keyword-only).  A time-dependent parameter's
    ``func`` takes the time as keyword-only ``t``.  Violations raise ``ValueError`` as in the
    reference (`tdgl/parameter.py:86-128`)."""

    def __init__(self, func: Callable, time_dependent: bool = False, **kwargs):
        kwargs.pop("use_cache", None)  # (reference option; nothing is cached here)
        spec = inspect.getfullargspec(func)
        args = spec.args
        n_pos = 2
        if args[:n_pos] != ["x", "y"]:
            raise ValueError(f"The first function arguments must be x and y, not {', '.join(args[:n_pos])!r}.")
        if "z" in args:
            if args.index("z") != n_pos:
                raise ValueError("If the function takes an argument z, it must be the third argument (x, y, z).")
            n_pos = 3
        defaults = spec.defaults or ()
        if len(defaults) != len(args) - n_pos:
            raise ValueError("All arguments other than x, y, z must be keyword arguments.")
        extra = set(kwargs) - set(args[n_pos:])
        if not extra.issubset(set(spec.kwonlyargs or [])):
            raise ValueError(f"Provided keyword-only arguments ({extra!r}) do not match the function signature: "
                             f"{function_repr(func)}.")
        if time_dependent and "t" not in (spec.kwonlyargs or []):
            raise ValueError("A time-dependent Parameter must take time t as a keyword argument.")
        if "t" in kwargs:
            raise ValueError("'t' cannot be bound as a Parameter keyword argument.")
        self.func = func
        self.time_dependent = bool(time_dependent)
        self.kwargs = dict(zip(args[n_pos:], defaults))
        self.kwargs.update(spec.kwonlydefaults or {})
        self.kwargs.update(kwargs)
        self._takes_z = n_pos == 3
        # True for factors that do not depend on position (e.g. LinearRamp): lets the solver
        # recognise A(t) = f(t) * A_static and keep A_static on the device
        self.uniform_in_space = False
        self.ramp = None  # LinearRamp: dict(tmin, tmax, initial, final)
        self.table = None  # TabulatedRamp: its PiecewiseLinear
        self.loop = None  # MovingCurrentLoop: dict(times, centers, currents, radius, unit_factor)

    def separable_product(self):
        """``(f, static)`` if this parameter is ``f(t) * static(x, y, z)`` with ``f`` uniform in
        space and ``static`` independent of time, else ``None``."""
        return None

    def separable_terms(self):
        """``(static_or_None, [(f_1, static_1), ..., (f_K, static_K)])`` if this parameter is a sum
        ``static + f_1(t) * static_1 + ... + f_K(t) * static_K`` the time loop can evaluate itself (see
        `CompositeParameter.separable_terms`), else ``None``.  A parameter that does not depend on time is the sum
        without products: ``(self, [])``."""
        return None if self.time_dependent else (self, [])

    def device_sources(self):
        """``(static_or_None, terms, loops)`` if this parameter is a sum of a static part, products the time loop
        evaluates (`separable_terms`) and `MovingCurrentLoop` leaves (see `CompositeParameter.device_sources`), else
        ``None``.  A `MovingCurrentLoop` by itself is ``(None, [], [its .loop])``."""
        if not self.time_dependent:
            return self, [], []
        return (None, [], [dict(self.loop)]) if getattr(self, "loop", None) is not None else None

    def scalar(self, t) -> float:
        """Value of a uniform-in-space factor at time ``t``."""
        z = np.zeros(1)
        return float(np.ravel(self(z, z, z, t=t))[0])

    def __call__(self, x, y, z=None, t=None):
        """Value at the points (arrays or numbers); the result is squeezed and a 0-d result
        returned as a number (`tdgl/parameter.py:156-172`)."""
        kw = dict(self.kwargs)
        if t is not None:
            kw["t"] = t
        elif self.time_dependent:
            kw["t"] = 0.0
        x, y = np.atleast_1d(x, y)
        if z is not None:
            if not self._takes_z:
                raise TypeError(f"{function_repr(self.func)} does not take z.")
            kw["z"] = np.atleast_1d(z)
        result = np.asarray(self.func(x, y, **kw)).squeeze()
        return result.item() if result.ndim == 0 else result

    def _clear_cache(self):  # reference API; nothing is cached here
        pass

    # -- arithmetic -------------------------------------------------------------------------------
    def __add__(self, other):
        return CompositeParameter(self, other, operator.add)

    def __radd__(self, other):
        return CompositeParameter(other, self, operator.add)

    def __sub__(self, other):
        return CompositeParameter(self, other, operator.sub)

    def __rsub__(self, other):
        return CompositeParameter(other, self, operator.sub)

    def __mul__(self, other):
        return CompositeParameter(self, other, operator.mul)

    def __rmul__(self, other):
        return CompositeParameter(other, self, operator.mul)

    def __truediv__(self, other):
        return CompositeParameter(self, other, operator.truediv)

    def __rtruediv__(self, other):
        return CompositeParameter(other, self, operator.truediv)

    def __pow__(self, other):
        return CompositeParameter(self, other, operator.pow)

    def __rpow__(self, other):
        return CompositeParameter(other, self, operator.pow)

    def __neg__(self):
        return CompositeParameter(-1.0, self, operator.mul)

    # -- identity ---------------------------------------------------------------------------------
    def __eq__(self, other) -> bool:
        """Same code, same bound arguments (`tdgl/parameter.py:246-275`)."""
        if other is self:
            return True
        if not isinstance(other, Parameter) or isinstance(other, CompositeParameter):
            return False
        if getattr(self.func, "__code__", self.func) != getattr(other.func, "__code__", other.func):
            return False
        if set(self.kwargs) != set(other.kwargs):
            return False
        return all(_same(self.kwargs[k], other.kwargs[k]) for k in self.kwargs)

    __hash__ = None

    def _argspec(self):
        names, values = list(self.kwargs), list(self.kwargs.values())
        if self.time_dependent:
            names.insert(0, "time_dependent")
            values.insert(0, True)
        return _BoundArgs(names, values)

    def _bare_repr(self) -> str:
        return function_repr(self.func, self._argspec())

    def __repr__(self):
        return f"{self.__class__.__name__}<{self._bare_repr()}>"

    def __getstate__(self):
        import cloudpickle

        state = self.__dict__.copy()
        state["func"] = cloudpickle.dumps(state["func"])  # (functions defined in a script or a test)
        return state

    def __setstate__(self, state):
        import cloudpickle

        state = dict(state)
        state["func"] = cloudpickle.loads(state["func"])
        self.__dict__.update(state)


class CompositeParameter(Parameter):
    """Result of ``+ - * / **`` between parameters and/or numbers (`tdgl/parameter.py:278-398`)."""

    VALID_OPERATORS = {operator.add: "+", operator.sub: "-", operator.mul: "*", operator.truediv: "/",
                       operator.pow: "**"}

    def __init__(self, left: Union[Number, Parameter], right: Union[Number, Parameter],
                 operator_: Union[Callable, str]):
        valid = (Number, Parameter)
        if not isinstance(left, valid):
            raise TypeError(f"Left must be a number, Parameter, or CompositeParameter, not {type(left)!r}.")
        if not isinstance(right, valid):
            raise TypeError(f"Right must be a number, Parameter, or CompositeParameter, not {type(right)!r}.")
        if isinstance(left, Number) and isinstance(right, Number):
            raise TypeError("Either left or right must be a Parameter or CompositeParameter.")
        if isinstance(operator_, str):
            operator_ = {v: k for k, v in self.VALID_OPERATORS.items()}.get(operator_.strip())
        if operator_ not in self.VALID_OPERATORS:
            raise ValueError(f"Unknown operator, {operator_!r}. Valid operators are {list(self.VALID_OPERATORS)!r}.")
        self.left, self.right, self.operator = left, right, operator_
        self.kwargs = {}
        self.time_dependent = any(isinstance(v, Parameter) and v.time_dependent for v in (left, right))
        self.uniform_in_space = all((not isinstance(v, Parameter)) or v.uniform_in_space for v in (left, right))
        self.ramp = self.table = None

    def separable_product(self):
        if self.operator is not operator.mul:
            return None
        for f, static in ((self.left, self.right), (self.right, self.left)):
            if (isinstance(f, Parameter) and f.uniform_in_space and f.time_dependent
                    and isinstance(static, Parameter) and not static.time_dependent):
                return f, static
        return None

    def separable_terms(self):
        """This parameter as ``A_0 + f_1(t) * A_1 + ... + f_K(t) * A_K``: ``(A_0 or None, [(f_k, A_k), ...])`` in the
        order the products appear, for a tree built from ``+`` and ``-`` whose leaves are parameters independent of
        time or products `separable_product` accepts with a `LinearRamp` or a `TabulatedRamp` as the factor.  The leaves
        independent of time fold into the one ``A_0``; a subtracted leaf enters with its static part negated (which is
        exact).  ``None`` when anything else appears in the tree -- a product of two factors, ``**``, a `Scale` with a
        function of its own, a bare number -- or when there are more than ``FIELD_TERMS_MAX`` products.  The value of the
        form, evaluated left to right as ``((A_0 + f_1 A_1) + f_2 A_2) + ...``, is what the time loop computes
        (`tdgl_set_link_terms`); it differs from ``self(x, y, z, t=t)`` by the rounding of a reordered sum only."""
        found = _collect_sum(self, loops=False)
        return None if found is None else found[:2]

    def device_sources(self):
        """`separable_terms` with moving loops: ``(A_0 or None, [(f_k, A_k), ...], [loop_1, ...])`` for a tree built from
        ``+`` and ``-`` whose leaves are what `separable_terms` accepts or a `MovingCurrentLoop`; each loop is its
        ``.loop`` dictionary, with the currents negated where the leaf is subtracted.  ``terms`` may be empty when
        ``loops`` is not.  ``None`` when anything else appears -- a loop times a ramp, for one --, for more than
        ``FIELD_TERMS_MAX`` products or more than ``FIELD_LOOPS_MAX`` loops.  The time loop evaluates the form as the
        terms' sum, left to right, then the loops in the order they appear (`tdgl_set_link_loops`)."""
        return _collect_sum(self, loops=True)

    def __call__(self, x, y, z=None, t=None):
        values = []
        for v in (self.left, self.right):
            if isinstance(v, Parameter):
                v = v(x, y, z, t=t) if v.time_dependent else v(x, y, z)
            values.append(v)
        a, b = values
        # a per-point scalar factor next to a vector field scales every component
        if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.ndim != b.ndim and a.ndim >= 1 and b.ndim >= 1:
            if a.ndim < b.ndim:
                a = a[:, None]
            else:
                b = b[:, None]
        return self.operator(a, b)

    def _bare_repr(self) -> str:
        side = lambda v: v._bare_repr() if isinstance(v, Parameter) else str(v)  # noqa: E731
        return f"({side(self.left)} {self.VALID_OPERATORS[self.operator]} {side(self.right)})"

    def __eq__(self, other) -> bool:
        if other is self:
            return True
        if not isinstance(other, CompositeParameter):
            return False
        return self.left == other.left and self.right == other.right and self.operator is other.operator

    __hash__ = None

    def __getstate__(self):
        return self.__dict__.copy()

    def __setstate__(self, state):
        self.__dict__.update(state)


FIELD_TERMS_MAX = 4  # products in a sum the time loop evaluates itself (TDGL_FIELD_TERMS_MAX)
FIELD_LOOPS_MAX = 2  # moving current loops on top of them (TDGL_FIELD_LOOPS_MAX)


def _collect_sum(p, loops: bool):
    """``(static or None, terms, loops)`` of the ``+`` / ``-`` tree under ``p``, the leaves independent of time folded left
    to right into the one static part; ``None`` where `_collect_terms` refuses the tree or it holds more than
    ``FIELD_TERMS_MAX`` products or ``FIELD_LOOPS_MAX`` loops.  Without ``loops`` a `MovingCurrentLoop` leaf is refused."""
    statics, terms, found = [], [], []
    if not _collect_terms(p, 1, statics, terms, found if loops else None) or len(terms) > FIELD_TERMS_MAX or len(found) > FIELD_LOOPS_MAX:
        return None
    static = None
    for leaf in statics:
        static = leaf if static is None else static + leaf
    return static, terms, found


def _collect_terms(p, sign: int, statics: list, terms: list, loops: Optional[list] = None) -> bool:
    """The leaves of the ``+`` / ``-`` tree under ``p`` into ``statics`` and ``terms`` (``separable_terms``), each with
    the sign it enters the sum with; False: the tree holds something the form does not cover.  With ``loops`` a list
    (``device_sources``) a `MovingCurrentLoop` leaf goes there, its currents carrying the sign."""
    if not isinstance(p, Parameter):
        return False
    signed = (lambda q: q) if sign > 0 else (lambda q: -q)  # noqa: E731
    if isinstance(p, CompositeParameter) and p.operator in (operator.add, operator.sub):
        right = sign if p.operator is operator.add else -sign
        return _collect_terms(p.left, sign, statics, terms, loops) and _collect_terms(p.right, right, statics, terms, loops)
    if not p.time_dependent:
        statics.append(signed(p))
        return True
    if loops is not None and getattr(p, "loop", None) is not None and not isinstance(p, CompositeParameter):
        loops.append(dict(p.loop, currents=sign * p.loop["currents"]))
        return True
    sep = p.separable_product()
    if sep is None or (sep[0].ramp is None and getattr(sep[0], "table", None) is None):
        return False
    terms.append((sep[0], signed(sep[1])))
    return True


class Constant(Parameter):
    """A parameter whose value depends on neither position nor time (`tdgl/parameter.py:417-438`)."""

    def __init__(self, value: Number, dimensions: int = 2):
        if dimensions not in (2, 3):
            raise ValueError(f"Dimensions must be 2 or 3, got {dimensions}.")
        if dimensions == 2:
            def constant(x, y, value=0):
                return value * np.ones_like(x)
        else:
            def constant(x, y, z, value=0):
                return value * np.ones_like(x)
        super().__init__(constant, value=value)
        self.uniform_in_space = True


# ---- sources (tdgl/sources/constant.py, scaling.py) ------------------------------------------
def constant_field_vector_potential(x, y, z, *, Bz):
    xs = x - (x.min() + np.ptp(x) / 2)
    ys = y - (y.min() + np.ptp(y) / 2)
    return np.stack([-Bz * ys / 2, Bz * xs / 2, np.zeros_like(xs)], axis=1)


def ConstantField(value: float = 0, field_units: str = "mT", length_units: str = "um") -> Parameter:
    """Vector potential of a uniform out-of-plane field ``value`` (in ``field_units``), in units
    of ``field_units * length_units`` (`tdgl/sources/constant.py:7-39`)."""

    return Parameter(constant_field_vector_potential, Bz=float(value))


def linear_ramp(x, y, z, *, t, tmin, tmax, initial=0.0, final=1.0):
    """``initial`` before ``tmin``, ``final`` after ``tmax``, linear in between -- one number for all
    positions (`tdgl/sources/scaling.py:4-14`)."""
    if t < tmin:
        return initial
    if t < tmax:
        return initial + (final - initial) * (t - tmin) / (tmax - tmin)
    return final


def LinearRamp(tmin: float = 0, tmax: float = 10, initial: float = 0, final: float = 1) -> Parameter:
    """A factor that ramps linearly from ``initial`` to ``final`` between ``tmin`` and ``tmax``
    (`tdgl/sources/scaling.py:17-40`)."""
    p = Parameter(linear_ramp, tmin=tmin, tmax=tmax, initial=initial, final=final, time_dependent=True)
    p.uniform_in_space = True
    p.ramp = dict(tmin=float(tmin), tmax=float(tmax), initial=float(initial), final=float(final))
    return p


def Scale(func, **kwargs) -> Parameter:
    """An arbitrary time-dependent scale factor ``func(x, y, z, *, t, **kwargs)``
    (`tdgl/sources/scaling.py:43-54`)."""
    kwargs["time_dependent"] = True
    return Parameter(func, **kwargs)


# ---- current loops (tdgl/sources/loop.py), static and moving ------------------------------------------------------------
LOOP_AGM_STEPS = 6  # halvings of the arithmetic-geometric mean: double precision down to 1 - m = 2e-9


def loop_potential_factor(dx, dy, dz, radius):
    """``H = G / rho`` of a circular loop of ``radius`` at the in-plane offsets ``dx, dy`` from its axis and the height
    ``dz != 0`` above its plane, so that ``A = mu_0 I H (-dy, dx)``.  ``G = ((2 - m) K(m) - 2 E(m)) d / (4 pi rho)`` with
    ``d^2 = (a + rho)^2 + dz^2``, ``m = 4 a rho / d^2`` is dimensionless and evaluated as the time loop's kernel does
    (`tdgl_set_link_loops`): ``(2 - m) K - 2 E = K sum_n 2^n c_n^2`` over the differences ``c_n`` of the
    arithmetic-geometric mean, every term positive, ``sqrt(1 - m)`` formed without ``1 - m``, ``c_0 / rho`` carried so
    that nothing is divided by ``rho``.  No elliptic integrals from a library, no angles."""
    dx, dy, dz = np.broadcast_arrays(np.asarray(dx, dtype=float), np.asarray(dy, dtype=float), np.asarray(dz, dtype=float))
    if np.any(dz == 0.0):
        raise ValueError("The loop's plane must differ from the plane of the points (z != loop z): the potential is "
                         "singular on the wire.")
    a = float(radius)
    rho = np.sqrt(dx * dx + dy * dy)
    z2, sp, sm = dz * dz, a + rho, a - rho
    d2 = sp * sp + z2
    b0 = np.sqrt((sm * sm + z2) / d2)
    ob = 1.0 + b0
    cr = (2.0 * a) / (d2 * ob)
    c = cr * rho
    an, bn, sr, p = 0.5 * ob, np.sqrt(b0), 2.0 * (cr * cr), 4.0
    with np.errstate(under="ignore"):
        for _ in range(LOOP_AGM_STEPS):
            a1 = 0.5 * (an + bn)
            bn = np.sqrt(an * bn)
            q = c / (4.0 * a1)
            cr, c = cr * q, c * q
            sr = sr + p * (cr * cr)
            p, an = p * 2.0, a1
    return (sr * np.sqrt(d2)) / (8.0 * an)


def loop_unit_factor(current_units: str, field_units: str, length_units: str) -> float:
    """``mu_0 I`` of a current of 1 ``current_units`` in ``field_units * length_units``."""
    from .device import CURRENT_UNITS, FIELD_UNITS, LENGTH_UNITS, MU_0, _unit

    return MU_0 * _unit(CURRENT_UNITS, current_units, "current") / (
        _unit(FIELD_UNITS, field_units, "field") * _unit(LENGTH_UNITS, length_units, "length"))


def _loop_potential(x, y, z, center, radius, amplitude):
    dx, dy = x - center[0], y - center[1]
    h = amplitude * loop_potential_factor(dx, dy, np.broadcast_to(z, np.shape(x)) - center[2], radius)
    return np.stack([-(dy * h), dx * h, np.zeros_like(h)], axis=1)


def loop_vector_potential(x, y, z, *, current, radius, center=(0, 0, 0), current_units="uA", field_units="mT",
                          length_units="um"):
    """``[n, 3]`` vector potential of a loop of current in ``field_units * length_units`` (`tdgl/sources/loop.py:9-33`)."""
    return _loop_potential(x, y, z, center, radius, current * loop_unit_factor(current_units, field_units, length_units))


def CurrentLoop(*, current: float, radius: float, center, current_units: str = "uA", field_units: str = "mT",
                length_units: str = "um") -> Parameter:
    """Vector potential of a circular loop of ``radius`` carrying ``current``, centred at ``center = (x, y, z)`` in a
    plane parallel to the film, in ``field_units * length_units`` (`tdgl/sources/loop.py:36-69`: the reference's
    signature and units).

    It deviates from the reference's values on purpose: the reference evaluates ``-(mu_0 I a / (pi m)) ((m - 2) K(m) +
    2 E(m)) / sqrt(denom)``, which cancels catastrophically for small ``m`` -- far from the loop and near its axis it has
    no correct digit below ``m ~ 1e-6``, and on the axis it is NaN.  Here the value is finite and correct everywhere off
    the wire, and exactly zero on the axis (`loop_potential_factor`).  The loop's plane must differ from the plane of
    the points, else ``ValueError``.  Static, so ``LinearRamp(...) * CurrentLoop(...)`` and ``ConstantField(b) +
    TabulatedRamp(...) * CurrentLoop(...)`` go to the device as terms."""
    loop_unit_factor(current_units, field_units, length_units)  # (unknown units are refused here)
    center = tuple(float(v) for v in center)
    if len(center) != 3:
        raise ValueError("center must be (x, y, z).")
    if not float(radius) > 0:
        raise ValueError("radius must be > 0.")
    return Parameter(loop_vector_potential, current=current, radius=radius, center=center, current_units=current_units,
                     field_units=field_units, length_units=length_units)


def moving_loop_vector_potential(x, y, z, *, t, times, centers, currents, radius, current_units="uA", field_units="mT",
                                 length_units="um"):
    """`loop_vector_potential` of the loop whose centre and current are piecewise linear in ``t`` on the nodes ``times``
    (constant outside)."""
    c = [float(np.interp(t, times, centers[:, j])) for j in range(3)]
    cur = float(np.interp(t, times, currents))
    return _loop_potential(x, y, z, c, radius, cur * loop_unit_factor(current_units, field_units, length_units))


def MovingCurrentLoop(times, centers, *, radius: float, current, current_units: str = "uA", field_units: str = "mT",
                      length_units: str = "um") -> Parameter:
    """A `CurrentLoop` that moves: ``A(r, t) = I(t) A_loop(r - c(t); radius)`` -- a susceptometer's field coil, a
    SQUID-on-tip or a magnetised tip scanned across the film, with or without a current waveform.  ``centers``
    ``[n_nodes, 3]`` and ``current`` (a number or ``[n_nodes]``) are piecewise linear in ``t`` on the shared ``times``
    and constant outside.  The loop's plane must stay on one side of the film.

    Called as a function it evaluates on the host.  Alone or in a sum with static fields, ramped or tabulated products
    and one more loop (`Parameter.device_sources`) the time loop evaluates it on the device (`tdgl_set_link_loops`): no
    Python call, no upload per step.  ``.loop`` holds ``dict(times, centers, currents, radius, unit_factor)``."""
    nodes = PiecewiseLinear(times, np.zeros(np.shape(times)))  # (its checks: one-dimensional, strictly increasing)
    centers = np.array(centers, dtype=float)
    if centers.shape != (len(nodes.times), 3):
        raise ValueError(f"centers must have shape (n_nodes, 3) = ({len(nodes.times)}, 3), got {centers.shape}.")
    currents = np.array(current, dtype=float) * np.ones(len(nodes.times)) if np.ndim(current) == 0 else np.array(current, dtype=float)
    if currents.shape != nodes.times.shape:
        raise ValueError(f"current must be a number or have shape (n_nodes,) = {nodes.times.shape}, got {currents.shape}.")
    if not (np.all(np.isfinite(centers)) and np.all(np.isfinite(currents)) and np.all(np.isfinite(nodes.times))):
        raise ValueError("times, centers and current must be finite.")
    if not float(radius) > 0:
        raise ValueError("radius must be > 0.")
    p = Parameter(moving_loop_vector_potential, times=nodes.times, centers=centers, currents=currents, radius=float(radius),
                  current_units=current_units, field_units=field_units, length_units=length_units, time_dependent=True)
    p.loop = dict(times=nodes.times, centers=centers, currents=currents, radius=float(radius),
                  unit_factor=loop_unit_factor(current_units, field_units, length_units))
    return p


# ---- tabulated time dependence, evaluated on the device ------------------------------------------
class PiecewiseLinear:
    """``f(t)``: linear between the nodes ``(times[k], values[k])``, constant outside.  Time-dependent
    inputs given in this form are uploaded once and evaluated by the time loop itself
    (`tdgl_set_mu_boundary_table` / `tdgl_set_epsilon_table`): no Python call, no upload per step."""

    def __init__(self, times, values):
        self.times = np.asarray(times, dtype=float)
        self.values = np.asarray(values, dtype=float)
        if self.times.ndim != 1 or self.times.shape != self.values.shape or len(self.times) < 1:
            raise ValueError("times and values must be one-dimensional and of equal length")
        if np.any(np.diff(self.times) <= 0):
            raise ValueError("times must increase strictly")

    def __call__(self, t) -> float:
        return float(np.interp(t, self.times, self.values))

    def __eq__(self, other) -> bool:
        return (isinstance(other, PiecewiseLinear) and np.array_equal(self.times, other.times)
                and np.array_equal(self.values, other.values))

    __hash__ = None


def tabulated_ramp(x, y, z, *, t, table):
    """The value of ``table`` at ``t`` -- one number for all positions."""
    return table(t)


def TabulatedRamp(times, values) -> Parameter:
    """A factor given as a table: linear between the nodes ``(times[k], values[k])``, constant before the first node
    and after the last (a `PiecewiseLinear`, kept as ``.table``).  ``TabulatedRamp(...) * <static field>`` is used
    exactly as ``LinearRamp(...) * <static field>`` is -- an up-and-down sweep, ramp-hold-ramp, a pulse, a sampled AC
    field -- and like it the time loop evaluates it on the device (`tdgl_set_link_table`): no Python call, no upload
    per step."""
    p = Parameter(tabulated_ramp, table=PiecewiseLinear(times, values), time_dependent=True)
    p.uniform_in_space = True
    p.table = p.kwargs["table"]
    return p


class TabulatedCurrents:
    """``terminal_currents`` as tables: ``TabulatedCurrents(times, dict(source=[...], drain=[...]))``.
    Callable like any ``t -> {name: current}`` function (so it works wherever the reference's
    callable does); the solver uploads the tables and the device evaluates them per step."""

    def __init__(self, times, currents):
        self.times = np.asarray(times, dtype=float)
        self.tables = {name: PiecewiseLinear(self.times, v) for name, v in currents.items()}

    def __call__(self, t):
        return {name: f(t) for name, f in self.tables.items()}

    def scaled(self, factor: float) -> "TabulatedCurrents":
        return TabulatedCurrents(self.times, {name: factor * f.values for name, f in self.tables.items()})


class SeparableEpsilon:
    """``disorder_epsilon(r, t) = factor(t) * static(r)``: ``static`` an array over the sites or a
    callable ``static(r[n, 2]) -> [n]``, ``factor`` a `PiecewiseLinear`.  Has the reference's calling
    convention (``epsilon(r, *, t, vectorized=True)``, `tdgl/solver/solver.py:191-216`); the solver
    keeps ``static`` on the device and evaluates ``factor`` inside the time loop."""

    def __init__(self, static, factor: PiecewiseLinear):
        self.static, self.factor = static, factor

    def static_values(self, sites) -> np.ndarray:
        s = self.static(np.asarray(sites)) if callable(self.static) else self.static
        return np.asarray(s, dtype=float) * np.ones(len(sites))

    def __call__(self, r, *, t=0.0, vectorized=True):
        return self.factor(t) * self.static_values(np.atleast_2d(r))


# ---- Gaussian hot spots in epsilon, evaluated on the device ---------------------------------------
EPS_SPOTS_MAX = 4  # TDGL_EPS_SPOTS_MAX


def table_value(times, values, t: float) -> float:
    """The library's ``table_value`` (csrc/kernels.inc) restated operation for operation: linear between the nodes,
    constant outside -- ``v[k-1] + (v[k] - v[k-1]) * ((t - t[k-1]) / (t[k] - t[k-1]))`` with ``t[k]`` the first node
    behind ``t``.  What host and device evaluate for every table; `np.interp` rounds differently."""
    t = float(t)
    if t <= times[0]:
        return float(values[0])
    if t >= times[-1]:
        return float(values[-1])
    hi = int(np.searchsorted(times, t, side="right"))
    t0, t1 = float(times[hi - 1]), float(times[hi])
    v0, v1 = float(values[hi - 1]), float(values[hi])
    return v0 + (v1 - v0) * ((t - t0) / (t1 - t0))


class HotSpot:
    """One Gaussian spot ``a(t) exp(-|r - c(t)|^2 / (2 sigma(t)^2))``: the centre, the amplitude ``a >= 0`` and the width
    ``sigma > 0`` at the nodes ``times`` (strictly increasing), each linear between the nodes and constant outside them.
    ``amplitudes`` and ``sigmas`` may be single numbers, ``centers`` a single point.  Lengths and time are those the solver
    hands to a ``disorder_epsilon``."""

    def __init__(self, times, centers, amplitudes, sigmas):
        self.times = np.atleast_1d(np.asarray(times, dtype=float))
        n = len(self.times)
        if self.times.ndim != 1 or n < 1:
            raise ValueError("HotSpot: times must be one-dimensional with at least one node.")
        centers = np.asarray(centers, dtype=float)
        if centers.shape == (2,):
            centers = np.broadcast_to(centers, (n, 2))
        self.centers = np.array(centers, dtype=float)
        amplitudes, sigmas = np.asarray(amplitudes, dtype=float), np.asarray(sigmas, dtype=float)
        if self.centers.shape != (n, 2):
            raise ValueError(f"HotSpot: centers must have shape (n_nodes, 2) = ({n}, 2), got {self.centers.shape}.")
        for name, v in (("amplitudes", amplitudes), ("sigmas", sigmas)):
            if v.shape not in ((), (n,)):
                raise ValueError(f"HotSpot: {name} must be a number or have shape (n_nodes,) = ({n},), got {v.shape}.")
        self.amplitudes = amplitudes * np.ones(n)
        self.sigmas = sigmas * np.ones(n)
        if not np.all(np.isfinite(self.times)) or np.any(np.diff(self.times) <= 0):
            raise ValueError("HotSpot: times must be finite and increase strictly.")
        if not np.all(np.isfinite(self.centers)):
            raise ValueError("HotSpot: centers must be finite.")
        if not (np.all(np.isfinite(self.amplitudes)) and np.all(self.amplitudes >= 0)):
            raise ValueError("HotSpot: amplitudes must be finite and >= 0.")
        # (sigma^2 a normal number: with a smaller one a site at the spot's centre would get 0 / 0)
        if not (np.all(np.isfinite(self.sigmas)) and np.all(self.sigmas > 0)
                and np.all(self.sigmas * self.sigmas >= np.finfo(float).tiny)):
            raise ValueError("HotSpot: sigmas must be finite and > 0, with a normal square.")

    def values(self, t: float) -> tuple:
        """``(cx, cy, a, sigma)`` at ``t``, by the library's `table_value`."""
        return tuple(table_value(self.times, v, t)
                     for v in (self.centers[:, 0], self.centers[:, 1], self.amplitudes, self.sigmas))


def hot_spot_epsilon(sites, eps0, values) -> np.ndarray:
    """``eps0 - sum_k a_k exp(-|r - c_k|^2 / (2 sigma_k^2))`` at ``values[k] = (cx, cy, a, sigma)``, with the library's
    operations in the library's order (k_eps_spots): all but ``exp`` are the same bits."""
    sites = np.asarray(sites, dtype=float)
    x, y = sites[:, 0], sites[:, 1]
    acc = np.array(eps0, dtype=float) * np.ones(len(sites))
    for cx, cy, a, s in values:
        dx, dy = x - float(cx), y - float(cy)
        d2 = dx * dx + dy * dy
        den = 2.0 * (float(s) * float(s))
        g = np.exp(-(d2 / den))
        acc = acc - float(a) * g
    return acc


class HotSpotEpsilon:
    """``disorder_epsilon(r, t) = static(r) - sum_k a_k(t) exp(-|r - c_k(t)|^2 / (2 sigma_k(t)^2))``: a local, moving,
    growing and fading suppression of the critical temperature -- a photon's hot spot in a nanowire detector, a laser spot
    scanned over a film, a heater pulse.  ``static`` (<= 1): a number, an array over the sites or a callable
    ``static(r[n, 2]) -> [n]`` (an array goes with the site array it was made for: a call at a single point or at another
    number of points raises); ``spots``: `HotSpot` s.  Has the reference's calling convention (``epsilon(r, *, t,
    vectorized=True)``), so it works wherever a callable does; with at most ``EPS_SPOTS_MAX`` spots the solver keeps
    ``static`` and the sites on the device and the time loop evaluates the spots itself (`tdgl_set_epsilon_spots`)."""

    def __init__(self, static=1.0, spots=()):
        self.static = static
        self.spots = [spots] if isinstance(spots, HotSpot) else list(spots)
        if not self.spots or not all(isinstance(s, HotSpot) for s in self.spots):
            raise ValueError("HotSpotEpsilon: spots must be a non-empty list of HotSpot.")

    def static_values(self, sites) -> np.ndarray:
        s = np.asarray(self.static(np.asarray(sites)) if callable(self.static) else self.static, dtype=float)
        if s.ndim > 0 and s.shape != (len(sites),):
            raise ValueError(f"HotSpotEpsilon: static has shape {s.shape}, but epsilon was asked at {len(sites)} point(s): an "
                             "array-valued static belongs to the whole site array (vectorized=True); use a number or a callable.")
        return s * np.ones(len(sites))

    def spot_values(self, t: float) -> list:
        return [s.values(t) for s in self.spots]

    def __call__(self, r, *, t=0.0, vectorized=True):
        r = np.asarray(r, dtype=float)
        out = hot_spot_epsilon(np.atleast_2d(r), self.static_values(np.atleast_2d(r)), self.spot_values(t))
        return out if r.ndim == 2 else float(out[0])
