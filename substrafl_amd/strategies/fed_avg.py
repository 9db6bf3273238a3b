"""FedAvg with the aggregation on MI355X.

Drop-in for ``substrafl.strategies.FedAvg`` (substrafl/strategies/fed_avg.py:23-274) on the
aggregation hot path: same class name, constructor, ``name``, ``@remote`` method
``avg_shared_states(shared_states) -> FedAvgAveragedState``, same exceptions, and results
bit-identical to the reference's NumPy arithmetic (fed_avg.py:217-222): the weighted sum of the
client buckets runs in libfedagg's HIP kernels (substrafl_amd/csrc/fedagg.hip).
"""

from typing import List, Optional

import numpy as np

from ..engine import Devices, check_downlink, check_robust, engine_for
from ..exceptions import EmptySharedStatesError
from ..remote import remote
from ..schemas import FedAvgAveragedState, FedAvgSharedState, StrategyName
from ..wire import has_topk
from .strategy import Strategy


def check_same_shapes(per_client_layers: List[List[np.ndarray]]) -> None:
    """``np.sum(list, axis=0)`` raises ValueError when the stacked arrays are inhomogeneous
    (fed_avg.py:222, scaffold.py:263/293)."""
    ref = per_client_layers[0]
    for other in per_client_layers[1:]:
        for a, b in zip(ref, other):
            if np.shape(a) != np.shape(b):
                raise ValueError(
                    "setting an array element with a sequence. The requested array has an inhomogeneous shape "
                    f"({np.shape(a)} vs {np.shape(b)})"
                )


class FedAvg(Strategy):
    """Federated averaging: ``Δw = Σ_k (n_k / n) Δw_k`` (fed_avg.py:23-52).

    ``downlink="mxfp8"`` (None, the default, changes nothing; any other string is a ``ValueError``):
    the average of clients on the MXFP8 or MXFP4 wire goes back to them encoded to MXFP8, 1.03 bytes
    per parameter instead of 4 (:meth:`engine.AggregationEngine.fedavg_mxfp8`); their
    ``weight_manager.increment_parameters`` decodes it on the device.  It carries no residual.

    ``robust="trimmed_mean"`` with ``trim`` in [0, 0.5), or ``robust="median"`` (None, the default,
    changes nothing; any other string is a ``ValueError``): the coordinate-wise trimmed mean, per
    element the ``floor(trim * K)`` lowest and highest of the K client values dropped and the rest
    averaged, or the median as its limit case (:meth:`engine.AggregationEngine.fedavg_robust`).  A
    client that sends NaN, Inf or a diverged update then no longer reaches the average.  The rule is
    **unweighted**: ``n_samples`` is validated as ever but every client has one vote.  ``trim`` is
    required for the trimmed mean (a bool, a non-number or a value outside [0, 0.5) is a
    ``ValueError``) and a ``TypeError`` with the median or without ``robust``.  Clients are untouched:
    the average comes back dense fp32.

    ``robust="krum"`` or ``robust="multi_krum"`` with ``byzantine=f`` (Blanchard et al. 2017): whole
    clients are selected by their pairwise distances, which catches an update that is an inlier in
    every coordinate but wrong as a vector (sign-flipped, colluding).  Krum returns the one client
    closest to its ``K - f - 2`` nearest neighbours, multi-Krum the unweighted average of the
    ``select`` best (default and at most ``K - f``); ``K >= 2 f + 3`` clients are needed (a
    ``ValueError`` when the states arrive).  ``byzantine`` is required (a bool, a non-int or a negative
    value is a ``ValueError``) and, like ``select`` outside multi-Krum, a ``TypeError`` with any other
    rule or without ``robust``."""

    def __init__(self, algo, metric_functions=None, device: Devices = None, downlink: Optional[str] = None,
                 robust: Optional[str] = None, trim: Optional[float] = None, byzantine: Optional[int] = None,
                 select: Optional[int] = None):
        check_downlink(downlink)
        check_robust(robust, trim, downlink, byzantine, select)
        extra = {k: v for k, v in (("device", device), ("downlink", downlink), ("robust", robust), ("trim", trim),
                                   ("byzantine", byzantine), ("select", select))
                 if v is not None}
        super().__init__(algo=algo, metric_functions=metric_functions, **extra)  # recorded only when given
        self._device = device
        self._downlink = downlink
        self._robust, self._trim = robust, trim
        self._byzantine, self._select = byzantine, select
        self._local_states = None
        self._shared_states = None

    @property
    def name(self) -> StrategyName:
        return StrategyName.FEDERATED_AVERAGING

    @remote
    def avg_shared_states(self, shared_states: List[FedAvgSharedState]) -> FedAvgAveragedState:
        """Weighted average of the clients' ``parameters_update`` by ``n_samples`` (fed_avg.py:176-224).

        Raises:
            EmptySharedStatesError: ``shared_states`` is empty (fed_avg.py:207-211).
            AssertionError: clients do not have the same number of layers (fed_avg.py:213-215).
            ZeroDivisionError: ``sum(n_samples) == 0`` (fed_avg.py:221).
            ValueError: a layer's shape differs between clients (``np.sum``, fed_avg.py:222).
            pydantic.ValidationError: a 0-d layer (its average is a scalar, schemas.py:29).
        """
        averaged_states = weighted_average(shared_states, "FedAvgSharedState", self._device, downlink=self._downlink,
                                           robust=self._robust, trim=self._trim, byzantine=self._byzantine,
                                           select=self._select)
        return FedAvgAveragedState(avg_parameters_update=averaged_states)


def weighted_average(shared_states, state_name: str, device: Devices = None, wire: bool = True,
                     empty_error=EmptySharedStatesError, downlink: Optional[str] = None,
                     robust: Optional[str] = None, trim: Optional[float] = None, byzantine: Optional[int] = None,
                     select: Optional[int] = None) -> List[np.ndarray]:
    """fed_avg.py:207-222 (also fed_pca.py:244-257): validation on the host, the weighted sum
    of every layer on the GPU.  ``wire``: layers in the flat wire format (this package's own
    schemas); False: plain NumPy arrays (the reference's schemas, :mod:`substrafl_amd.integration`).
    ``empty_error``: the exception class raised for an empty list (the reference's own there).
    ``downlink``: FedAvg's option, passed to the engine's ``fedavg_routed`` when set.  ``robust`` /
    ``trim``: FedAvg's options; when ``robust`` is set the engine's ``fedavg_robust`` reduces the layers
    by the unweighted trimmed mean or median instead (``n_samples`` is validated but not used);
    ``byzantine`` / ``select``: the options of its rules ``"krum"`` and ``"multi_krum"``."""
    if len(shared_states) == 0:
        raise empty_error(
            "Your shared_states is empty. Please ensure that "
            f"the train method of your algorithm returns a {state_name} object."
        )
    parameters_update_len = len(shared_states[0].parameters_update)
    assert all(
        [len(shared_state.parameters_update) == parameters_update_len for shared_state in shared_states]
    ), "Not the same number of layers for every input parameters."

    n_samples = [state.n_samples for state in shared_states]
    n_all_samples = sum(n_samples)
    if parameters_update_len == 0:
        return []
    if n_all_samples == 0:
        raise ZeroDivisionError("division by zero")
    updates = [list(state.parameters_update) for state in shared_states]
    if not any(has_topk(u) for u in updates):  # top-k rows differ in length: the engine compares their shape tables
        check_same_shapes(updates)
    engine = engine_for(device)
    if robust is not None:
        check_robust(robust, trim, downlink, byzantine, select)
        if byzantine is None:
            return engine.fedavg_robust(updates, robust, trim, wire=wire)
        return engine.fedavg_robust(updates, robust, trim, wire=wire, byzantine=byzantine, select=select)
    # substrafl_amd's own schemas already need this package to unpickle: the flat wire format.
    # fedavg_routed where the engine has it: fedavg, plus wire.BF16 states on the multi-GPU and
    # out-of-core routes, which fedavg itself refuses
    if downlink is not None:
        return engine.fedavg_routed(updates, n_samples, wire=wire, downlink=downlink)
    return getattr(engine, "fedavg_routed", engine.fedavg)(updates, n_samples, wire=wire)
