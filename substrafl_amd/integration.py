"""The drop-in for SubstraFL's experiment drivers: the reference's own strategy classes with their
aggregation method bodies on the MI355X engine.

``accelerate(substrafl.strategies.FedAvg)`` returns a subclass of the reference class that keeps
everything of it -- constructor, ``name``, graph building (``build_compute_plan``,
``perform_round``; substrafl/strategies/fed_avg.py:79-137, strategy.py:183-246), the reference's
``@remote`` decorator and schemas -- and replaces only the bodies of the aggregation methods:

* ``FedAvg.avg_shared_states`` (fed_avg.py:176-224): the weighted sum of the client layers in
  ``fedavg_kernel`` (bit-identical to fed_avg.py:217-222);
* ``Scaffold.avg_shared_states`` (scaffold.py:297-337): the fp64 two-bucket reduction, ``c`` last
  and ``aggregation_lr`` after the sum, with the ``c`` equality check of scaffold.py:193-196
  counted while ``c`` is staged;
* ``FedPCA.avg_shared_states`` / ``avg_shared_states_with_qr`` (fed_pca.py:210-299): FedAvg's
  reduction (+ the reference's ``np.linalg.qr`` of each averaged matrix; opt-in,
  ``accelerate(FedPCA, qr="device")`` or ``FEDAGG_PCA_QR=device``: an fp64 Householder LQ on the GPU
  instead, held to error bounds);
* ``NewtonRaphson.compute_averaged_states`` (newton_raphson.py:151-216): the weighted sums of the
  clients' Hessians and gradients (the explicit ``+=`` chain, ``engine.sequential_sum``), then the
  reference's own ``np.linalg.solve`` and unflatten on the host.  Opt-in, ``accelerate(NewtonRaphson,
  solve="device")`` or ``FEDAGG_NR_SOLVE=device``: the dense solve on the GPU too (fp64 LU with
  partial pivoting, ``libfedagg_dense.so``), held to backward-error bounds instead of LAPACK's bits
  (include/fedagg_dense.h); ``solve="cholesky"``: a Cholesky solve there for a Hessian sum
  that is symmetric positive definite, that LU for any other; the default is unchanged.

The client half of NewtonRaphson ends every round with an eigenvalue check of its Hessian
(torch_newton_raphson_algo.py:346-352); :func:`newton_raphson_hessian_check` restates it with an
opt-in Cholesky certificate on the GPU ahead of it (``accelerate_algo(TorchNewtonRaphsonAlgo,
hessian_check="device")`` or ``FEDAGG_NR_CHECK=device``).

So the class goes straight into ``simulate_experiment`` / ``execute_experiment``::

    from substrafl.strategies import FedAvg
    from substrafl_amd.integration import accelerate

    strategy = accelerate(FedAvg)(algo=my_algo)      # same arguments as the reference class

Error behaviour is the reference's: its ``EmptySharedStatesError``, the layer-count
``AssertionError``, ``ZeroDivisionError`` for ``sum(n_samples) == 0``, ``ValueError`` for shapes
that differ between clients, ``AssertionError`` for differing server control variates.  The task
process re-creates the strategy from its ``RemoteStruct`` (``cls=self.__class__``): cloudpickle
carries the generated subclass by value, so the task environment needs ``substrafl_amd`` (with its
built ``libfedagg.so``) next to ``substrafl``.  Nothing here imports SubstraFL at module level.
"""

from __future__ import annotations

import importlib
import os
from typing import Optional

import numpy as np

from . import handoff
from .engine import Devices, engine_for
from .strategies.fed_avg import check_same_shapes, weighted_average
from .strategies.fed_pca import orthonormal_layers
from .strategies.scaffold import Scaffold as _MirrorScaffold
from .strategies.strategy import Strategy as _MirrorStrategy


def _reference_modules(strategy_cls):
    """The reference package the class comes from (``substrafl``): its strategies, schemas,
    ``remote`` decorator and exceptions.  Found from the first class in the MRO that lives in a
    ``<pkg>.strategies`` module, so a user subclass defined anywhere (``__main__``) works."""
    mods = [b.__module__ for b in getattr(strategy_cls, "__mro__", ())]
    pkg = next((m.split(".")[0] for m in mods if ".strategies" in m), strategy_cls.__module__.split(".")[0])
    return (importlib.import_module(f"{pkg}.strategies"), importlib.import_module(f"{pkg}.strategies.schemas"),
            importlib.import_module(f"{pkg}.remote").remote, importlib.import_module(f"{pkg}.exceptions"))


def _solve_mode(solve: str) -> str:
    """``solve`` (``"host"``, ``"device"`` or ``"cholesky"``) under the environment override
    ``FEDAGG_NR_SOLVE``."""
    return _check_solve(os.environ.get("FEDAGG_NR_SOLVE") or solve)


def _check_solve(solve: str) -> str:
    if solve not in ("host", "device", "cholesky"):
        raise ValueError(f"solve must be 'host', 'device' or 'cholesky', not {solve!r}")
    return solve


def accelerate(strategy_cls, device: Devices = None, solve: str = "host", qr: str = "host"):
    """A subclass of the reference strategy class ``strategy_cls`` (``FedAvg``, ``Scaffold``,
    ``FedPCA``, ``NewtonRaphson`` or a subclass of one of them) whose aggregation methods run on the
    engine of ``device`` (:func:`engine.engine_for`: None = the current GPU, an index, a list, or
    "all").  ``solve`` matters for NewtonRaphson only: ``"host"`` (the default) keeps the
    reference's ``np.linalg.solve``, bit for bit; ``"device"`` solves the Newton system on the GPU
    as well, by LU with partial pivoting; ``"cholesky"`` tries a Cholesky factorisation there first
    and keeps the LU for a sum that is not symmetric positive definite (:func:`newton_raphson_update`).
    ``FEDAGG_NR_SOLVE=cholesky|device|host`` overrides it, read when the aggregation runs.  ``qr``
    matters for FedPCA only: ``"host"`` (the default) keeps the reference's ``np.linalg.qr`` of each
    averaged matrix, bit for bit; ``"device"`` orthonormalises each one on the GPU (:func:`strategies.fed_pca.orthonormal_layers`).  ``FEDAGG_PCA_QR=device|host``
    overrides it, read when the aggregation runs."""
    _check_solve(solve)
    if qr not in ("host", "device"):
        raise ValueError(f"qr must be 'host' or 'device', not {qr!r}")
    strategies, schemas, remote, exceptions = _reference_modules(strategy_cls)
    empty = exceptions.EmptySharedStatesError
    base_init = strategy_cls.__init__

    def __init__(self, *args, **kwargs):
        base_init(self, *args, **kwargs)
        handoff.register("aggregator", self)  # the clients' exports are recorded for it (handoff.py)

    ns = {"__doc__": f"{strategy_cls.__name__} with its aggregation on MI355X (substrafl_amd.integration).",
          "__init__": __init__,
          "_fedagg_device": device,
          # the task-process hooks of INTEGRATION.md §3 (prewarm, overlapped ingest), as the mirrors have them
          "prewarm_aggregation": _MirrorStrategy.prewarm_aggregation,
          "ingest_shared_states": _MirrorStrategy.ingest_shared_states}

    if issubclass(strategy_cls, strategies.Scaffold):
        averaged_cls = schemas.ScaffoldAveragedStates

        def avg_shared_states(self, shared_states):
            """scaffold.py:297-337 on the engine (``c`` check of :193-196 while ``c`` is staged)."""
            new_c, avg = scaffold_average(self, shared_states, self._aggregation_lr, self._fedagg_device)
            return averaged_cls(server_control_variate=new_c, avg_parameters_update=avg)

        ns["avg_shared_states"] = remote(avg_shared_states)
        ns["_aggregation_methods"] = {"avg_shared_states": "scaffold"}
    elif issubclass(strategy_cls, strategies.FedPCA):
        averaged_cls = schemas.FedPCAAveragedState

        def avg_shared_states(self, shared_states):
            """fed_pca.py:210-259 (FedAvg's reduction) on the engine."""
            out = weighted_average(shared_states, "FedPCASharedState", self._fedagg_device, wire=False,
                                   empty_error=empty)
            return averaged_cls(avg_parameters_update=out)

        def avg_shared_states_with_qr(self, shared_states):
            """fed_pca.py:261-299: the average on the engine, then the reference's QR per layer
            (``qr="host"``) or the fp64 Householder LQ on the device (``qr="device"``)."""
            out = weighted_average(shared_states, "FedPCASharedState", self._fedagg_device, wire=False,
                                   empty_error=empty)
            return averaged_cls(avg_parameters_update=orthonormal_layers(out, self._fedagg_device, self._fedagg_qr))

        ns["_fedagg_qr"] = qr
        ns["avg_shared_states"] = remote(avg_shared_states)
        ns["avg_shared_states_with_qr"] = remote(avg_shared_states_with_qr)
        ns["_aggregation_methods"] = {"avg_shared_states": "fedavg", "avg_shared_states_with_qr": "fedavg"}
    elif issubclass(strategy_cls, strategies.FedAvg):
        averaged_cls = schemas.FedAvgAveragedState

        def avg_shared_states(self, shared_states):
            """fed_avg.py:176-224 on the engine."""
            out = weighted_average(shared_states, "FedAvgSharedState", self._fedagg_device, wire=False,
                                   empty_error=empty)
            return averaged_cls(avg_parameters_update=out)

        ns["avg_shared_states"] = remote(avg_shared_states)
        ns["_aggregation_methods"] = {"avg_shared_states": "fedavg"}
    elif getattr(strategies, "NewtonRaphson", None) is not None and issubclass(strategy_cls, strategies.NewtonRaphson):
        averaged_cls = schemas.NewtonRaphsonAveragedStates

        def compute_averaged_states(self, shared_states):
            """newton_raphson.py:151-216: the reference's checks, the two weighted sums on the
            engine, then the reference's own dense solve on the host (``solve="host"``) or the
            fp64 LU on the device (``solve="device"``; ``solve="cholesky"``: a Cholesky ahead of it),
            and the reference's unflatten."""
            self._check_shared_states(shared_states)
            update = newton_raphson_update(shared_states, self._damping_factor, self._fedagg_device,
                                           solve=self._fedagg_solve)
            return averaged_cls(parameters_update=self._unflatten_array(update, shared_states[-1].gradients))

        ns["_fedagg_solve"] = solve
        ns["compute_averaged_states"] = remote(compute_averaged_states)
        ns["_aggregation_methods"] = {"compute_averaged_states": "sequential"}
    else:
        raise TypeError(f"accelerate takes SubstraFL's FedAvg, Scaffold, FedPCA or NewtonRaphson (or a subclass), "
                        f"not {strategy_cls!r}")
    cls = type(strategy_cls.__name__, (strategy_cls,), ns)
    # not importable by name: cloudpickle carries the class by value into the task process
    cls.__qualname__ = f"accelerate.<locals>.{strategy_cls.__name__}"
    return cls


def _newton_raphson_rows(shared_states):
    """``(hessians, gradients, n_samples)`` as :meth:`engine.AggregationEngine.sequential_sum` takes
    them, after the reference's host-side errors (newton_raphson.py:195-211)."""
    n_samples = [s.n_samples for s in shared_states]
    if sum(int(n) for n in n_samples) == 0:
        raise ZeroDivisionError("division by zero")  # n_samples / n_all_samples (:201)
    hessians = [[np.asarray(s.hessian)] for s in shared_states]
    gradients = [[np.concatenate([np.asarray(g).reshape(-1) for g in s.gradients])] for s in shared_states]
    check_same_shapes(hessians)  # total_hessians += ... (:208)
    check_same_shapes(gradients)
    return hessians, gradients, n_samples


def newton_raphson_update(shared_states, damping_factor, device: Optional[Devices] = None, solve: str = "device"):
    """The flat parameter update of NewtonRaphson.compute_averaged_states (newton_raphson.py:195-213),
    ``-damping_factor * solve(sum_k c_k H_k, sum_k c_k g_k)``, for any strategy object or host.

    ``solve="host"``: :func:`newton_raphson_sums`, then ``np.linalg.solve`` -- the reference's bits.
    ``solve="device"``: the sums stay in HBM and ``fedagg_dense_solve_f64`` solves the system there
    (:meth:`engine.AggregationEngine.newton_raphson_solve`); only the P doubles of ``x`` come home.
    The sums are the same bits either way; ``x`` is then within the backward-error bounds of
    include/fedagg_dense.h instead of LAPACK's rounding, and deterministic run to run.  The device
    route needs a float64 Hessian sum and a float32 or float64 gradient sum; anything else (an fp32
    Hessian, which NumPy solves in single precision; fp16, which it refuses) takes the host solve
    and says why in ``last_timing["solve"]``.  An exactly-zero pivot raises NumPy's
    ``LinAlgError("Singular matrix")``.  NaN or Inf in the inputs raise nothing, as with NumPy;
    what they give is unspecified.  ``FEDAGG_NR_SOLVE`` overrides ``solve``.

    ``solve="cholesky"``: the device route with ``method="cholesky"``.  A Hessian sum that equals its
    transpose by value and whose Cholesky factorisation runs to completion (``fedagg_dense_potrf_f64``,
    ``info == 0``) is solved from that factor (``fedagg_dense_potrs_f64``): ``x`` then satisfies
    ``|b - A x| <= gamma_{3n+1} |L| |L^T| |x|`` (include/fedagg_dense.h), and ``last_timing["solve"]``
    is ``"device: cholesky"``.  Any other sum gets the LU of ``solve="device"``, bit for bit, after the
    failed attempt, and ``last_timing["solve"]`` says which of the two it was.  No shift and no
    tolerance: the Cholesky answer is only ever taken from a factorisation that ran to completion."""
    mode = _solve_mode(solve)
    hessians, gradients, n_samples = _newton_raphson_rows(shared_states)
    eng = engine_for(device)
    eng = eng._single() if hasattr(eng, "_single") else eng  # several GPUs: the first one, as for the sums
    reason = "host"
    if mode != "host":
        if mode == "device":  # (without the keyword: an engine stand-in of before it still fits)
            x, info, reason = eng.newton_raphson_solve(hessians, gradients, n_samples)
        else:
            x, info, reason = eng.newton_raphson_solve(hessians, gradients, n_samples, method="cholesky")
        if x is not None:
            if info != 0:
                raise np.linalg.LinAlgError("Singular matrix")
            return -damping_factor * x
    (total_h,) = eng.sequential_sum(hessians, n_samples)
    (total_g,) = eng.sequential_sum(gradients, n_samples)
    update = -damping_factor * np.linalg.solve(total_h, total_g)
    if isinstance(getattr(eng, "last_timing", None), dict):  # (an engine stand-in may keep no timing)
        eng.last_timing["solve"] = reason
    return update


def newton_raphson_sums(shared_states, device: Optional[Devices] = None):
    """The weighted Hessian and gradient sums of NewtonRaphson.compute_averaged_states
    (newton_raphson.py:195-211) on the engine (:meth:`engine.AggregationEngine.sequential_sum`:
    the explicit ``+=`` chain from client 0's product, bit for bit).  Returns ``(total_hessians,
    total_gradient_one_d)``; the gradients are concatenated per client first, as there.
    ``ZeroDivisionError`` for ``sum(n_samples) == 0`` and ``ValueError`` for sizes that differ
    between clients, before any device work."""
    hessians, gradients, n_samples = _newton_raphson_rows(shared_states)
    eng = engine_for(device)
    (total_h,) = eng.sequential_sum(hessians, n_samples)
    (total_g,) = eng.sequential_sum(gradients, n_samples)
    return total_h, total_g


def _check_mode(check: str) -> str:
    """``check`` (``"host"`` or ``"device"``) under the environment override ``FEDAGG_NR_CHECK``."""
    mode = os.environ.get("FEDAGG_NR_CHECK") or check
    if mode not in ("host", "device"):
        raise ValueError(f"check must be 'host' or 'device', not {mode!r}")
    return mode


# the route the last newton_raphson_hessian_check of this process took ("route"), with the engine's
# timing of the device part when it ran ("timing")
last_hessian_check: dict = {}


def newton_raphson_hessian_check(hessian, l2_coeff, device: Optional[Devices] = None, check: str = "device",
                                 error_cls=None):
    """The convexity check at the end of TorchNewtonRaphsonAlgo.train
    (torch_newton_raphson_algo.py:346-352): raise ``error_cls`` (default
    :class:`substrafl_amd.exceptions.NegativeHessianMatrixError`) unless every eigenvalue of
    ``hessian`` is >= 0.  Returns the route taken, also left in ``last_hessian_check["route"]``.

    ``check="host"``: the reference's lines as they are -- ``np.linalg.eig``, the real parts, the
    message with the eigenvalue list and ``l2_coeff``.  Route ``"host"``.

    ``check="device"``: a Cholesky factorisation on the GPU first
    (:meth:`engine.AggregationEngine.hessian_cholesky_check`, ``fedagg_dense_potrf_f64``).  One that
    runs to completion proves ``H + E`` positive definite for an ``E`` with ``|E| <=
    gamma_{n+1} |L| |L^T|`` (include/fedagg_dense.h), and the Hessian is accepted: route
    ``"device"``, no eigenvalue is computed.  A failed pivot (``info = j``: route ``"host after
    device info=j"``) or a Hessian the engine declines (not float64, not square, not exactly
    symmetric: the route is the engine's reason, ``"host: ..."``) proves nothing either way, and the
    reference's host rule decides, raising with the reference's message.  The device therefore only
    ever accepts; it never raises by itself.

    The one divergence from the reference: a matrix whose smallest eigenvalue lies within the
    factorisation's backward error below zero may be accepted on the device where ``dgeev`` reports
    a negative eigenvalue -- a band in which ``dgeev``'s own sign is rounding noise as well.  No
    shift or tolerance is applied.  ``FEDAGG_NR_CHECK=device|host`` overrides ``check``."""
    mode = _check_mode(check)
    route, timing = "host", None
    if mode == "device":
        eng = engine_for(device)
        eng = eng._single() if hasattr(eng, "_single") else eng  # several GPUs: the first one
        ok, info, reason = eng.hessian_cholesky_check(hessian)
        timing = getattr(eng, "last_timing", None) if ok is not None else None
        route = reason if ok is None else "device" if ok else f"host after device info={info}"
        if isinstance(timing, dict):  # (an engine stand-in may keep no timing)
            timing["check"] = route
    last_hessian_check.clear()
    last_hessian_check.update({"route": route, "timing": timing})
    if route == "device":
        return route
    eigenvalues = np.linalg.eig(hessian)[0].real
    if not (eigenvalues >= 0).all():
        if error_cls is None:
            from .exceptions import NegativeHessianMatrixError as error_cls
        raise error_cls(
            "Hessian matrix is not positive semi-definite, either the problem is not convex or due to numerical"
            " instability. It is advised to try to increase the l2_coeff. "
            f"Calculated eigenvalues are {eigenvalues.tolist()} and considered l2_coeff is {l2_coeff}")
    return route


def accelerate_algo(algo_cls, wire: bool = False, hessian_check: Optional[str] = None):
    """The client half: :func:`substrafl_amd.algorithms.accelerate.accelerate_algo`.
    Imported on call, so the aggregation side of this module never imports torch."""
    from .algorithms.accelerate import accelerate_algo as _accelerate_algo

    return _accelerate_algo(algo_cls, wire=wire, hessian_check=hessian_check)


def scaffold_average(strategy, shared_states, aggregation_lr, device: Optional[Devices] = None, wire: bool = False):
    """Scaffold.avg_shared_states' arithmetic (scaffold.py:297-337) for any strategy object:
    the checks of scaffold.py:168-202 (element-wise ``c`` equality counted by the engine), then
    ``(new_server_control_variate, avg_parameters_update)``, both fp64."""
    _MirrorScaffold._check_shared_states(strategy, shared_states=shared_states)
    cvs = [list(s.control_variate_update) for s in shared_states]
    pus = [list(s.parameters_update) for s in shared_states]
    c0 = list(shared_states[0].server_control_variate)
    check_same_shapes([*cvs, c0])  # np.sum([w*cv_k ..., c]) (scaffold.py:263)
    check_same_shapes(pus)  # np.sum([w*Δ_k ...]) (scaffold.py:293)
    engine = engine_for(device)
    # kinds per bucket where the engine has them (16-bit buckets, on one GPU or range-sharded over
    # several), else one kind per call
    mismatches, new_c, avg = getattr(engine, "scaffold_per_bucket", engine.scaffold)(
        pus, cvs, _MirrorScaffold._server_control_variates(shared_states), [s.n_samples for s in shared_states],
        aggregation_lr, wire=wire)
    assert mismatches == 0, "all server_control_variate in the shared_states are not equal"
    return new_c, avg
