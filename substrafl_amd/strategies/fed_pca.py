"""FedPCA's aggregation on MI355X (kernel reuse).

``FedPCA.avg_shared_states`` (substrafl/strategies/fed_pca.py:210-259) is, operation for
operation, FedAvg's weighted average (fed_avg.py:217-222), so it runs on the
same bucket kernel and is bit-identical to the reference.  ``avg_shared_states_with_qr``
(:261-299) averages on the GPU the same way and then factorises each averaged matrix with
``np.linalg.qr`` exactly as the reference does -- the QR is a small dense LAPACK call on the
result, not part of the element-wise hot path.  Opt-in, ``FedPCA(...,
qr="device")`` or ``FEDAGG_PCA_QR=device``: each averaged matrix is orthonormalised on the GPU as
well (:func:`orthonormal_layers`: fp64 Householder LQ, ``libfedagg_dense.so``), held to error bounds
instead of LAPACK's bits (include/fedagg_dense.h); the default is unchanged.  The federated-PCA
graph building (``perform_round``) is Substra control plane and out of scope.
"""

import os
from typing import List, Optional

import numpy as np

from ..engine import Devices, engine_for
from ..remote import remote
from ..schemas import FedPCAAveragedState, FedPCASharedState, StrategyName
from .fed_avg import weighted_average
from .strategy import Strategy


def qr_mode(qr: str) -> str:
    """``qr`` (``"host"`` or ``"device"``) under the environment override ``FEDAGG_PCA_QR``."""
    mode = os.environ.get("FEDAGG_PCA_QR") or qr
    if mode not in ("host", "device"):
        raise ValueError(f"qr must be 'host' or 'device', not {mode!r}")
    return mode


def orthonormal_layers(averaged, device: Devices = None, qr: str = "host") -> List[np.ndarray]:
    """fed_pca.py:289-299 for every layer ``a`` of the averaged state: ``np.linalg.qr(a.T)[0].T``.

    ``qr="host"``: exactly that line, the reference's bits.  ``qr="device"``: each layer goes through
    :meth:`engine.AggregationEngine.orthonormal_rows` (``fedagg_dense_gelqf_f64`` +
    ``fedagg_dense_orglq_f64``; an fp32 layer is factored in fp64 and rounded, as NumPy does); a
    layer the engine declines (not a 2-D float32 / float64 matrix with ``n <= m``) takes the host
    line as today.  The route of the last layer is left in the engine's ``last_timing["qr"]``, those
    of all layers in ``last_timing["qr_layers"]``.  ``FEDAGG_PCA_QR`` overrides ``qr``, read here."""
    if qr_mode(qr) == "host":
        return [np.linalg.qr(a.T)[0].T for a in averaged]  # fed_pca.py:295-296
    eng = engine_for(device)
    eng = eng._single() if hasattr(eng, "_single") else eng  # several GPUs: the first one
    out, routes = [], []
    for a in averaged:
        q, reason = eng.orthonormal_rows(a)
        routes.append(reason)
        if isinstance(getattr(eng, "last_timing", None), dict):  # (an engine stand-in may keep no timing)
            eng.last_timing["qr"] = reason
        out.append(np.linalg.qr(a.T)[0].T if q is None else q)  # (the host line may raise, as today)
    if isinstance(getattr(eng, "last_timing", None), dict):
        eng.last_timing["qr_layers"] = routes
    return out


class FedPCA(Strategy):
    _aggregation_methods = {"avg_shared_states": "fedavg", "avg_shared_states_with_qr": "fedavg"}

    def __init__(self, algo, metric_functions=None, device: Devices = None, qr: str = "host"):
        if qr not in ("host", "device"):
            raise ValueError(f"qr must be 'host' or 'device', not {qr!r}")
        # only what differs from the default is recorded for the task process's re-creation
        extra = {}
        if device is not None:
            extra["device"] = device
        if qr != "host":
            extra["qr"] = qr
        super().__init__(algo=algo, metric_functions=metric_functions, **extra)
        self._device = device
        self._qr = qr
        self._local_states = None
        self._shared_states = None

    @property
    def name(self) -> StrategyName:
        return StrategyName.FEDERATED_PCA

    @remote
    def avg_shared_states(self, shared_states: List[FedPCASharedState]) -> FedPCAAveragedState:
        averaged = weighted_average(shared_states, "FedPCASharedState", self._device)
        return FedPCAAveragedState(avg_parameters_update=averaged)

    @remote
    def avg_shared_states_with_qr(self, shared_states: List[FedPCASharedState]) -> FedPCAAveragedState:
        averaged = weighted_average(shared_states, "FedPCASharedState", self._device)
        out = orthonormal_layers(averaged, self._device, getattr(self, "_qr", "host"))
        return FedPCAAveragedState(avg_parameters_update=out)
