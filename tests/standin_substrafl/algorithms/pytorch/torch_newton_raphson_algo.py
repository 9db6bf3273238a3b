"""NewtonRaphson's client: apply the averaged update, make one pass over every sample while the
loss's gradient and Hessian accumulate on the host in float64, refuse a Hessian with a negative
eigenvalue, return both (the reference's ``TorchNewtonRaphsonAlgo.train`` sequence and attribute
names), written for this stand-in in per-layer torch ops."""

import math

import numpy as np
import torch

from ...remote import remote_data
from ...strategies.schemas import NewtonRaphsonSharedState, StrategyName
from . import _weights as w
from .torch_base_algo import TorchAlgo


class NegativeHessianMatrixError(Exception):
    """The accumulated Hessian has a negative eigenvalue."""


class _OnePass:
    """Batch sampler of one pass in order, the last batch short: every sample exactly once, with
    the counters ``train`` reads (``n_samples``, ``reset_counter``, ``check_num_updates``)."""

    def __init__(self, n_samples: int, batch_size):
        self.n_samples = int(n_samples)
        self.batch_size = self.n_samples if batch_size is None else int(batch_size)
        self.num_updates = math.ceil(self.n_samples / self.batch_size)
        self.counter = 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.counter == self.num_updates:
            raise StopIteration
        lo = self.counter * self.batch_size
        self.counter += 1
        return list(range(lo, min(lo + self.batch_size, self.n_samples)))

    def reset_counter(self):
        self.counter = 0

    def check_num_updates(self):
        assert self.counter == self.num_updates, (self.counter, self.num_updates)


class TorchNewtonRaphsonAlgo(TorchAlgo):
    def __init__(self, model, criterion, batch_size, dataset, l2_coeff: float = 0,
                 with_batch_norm_parameters: bool = False, disable_gpu: bool = False, *args, **kwargs):
        assert "optimizer" not in kwargs
        super().__init__(model, criterion, None, dataset, None, None, disable_gpu, *args, **kwargs)
        assert criterion.reduction == "mean"
        self._with_batch_norm_parameters = with_batch_norm_parameters
        self._l2_coeff = l2_coeff
        self._batch_size = batch_size
        self._final_gradients = self._final_hessian = self._n_samples_done = None

    @property
    def strategies(self):
        return [StrategyName.NEWTON_RAPHSON]

    def _instantiate_index_generator(self, n_samples):
        return _OnePass(n_samples, self._batch_size)

    def _initialize_gradients_and_hessian(self):
        params = list(self._model.parameters())
        size = sum(p.numel() for p in params if p.requires_grad)
        return [np.zeros(tuple(p.shape), np.float32) for p in params], np.zeros((size, size)), 0

    def _derivatives(self, values):
        """d values[i] / d parameter, one entry per (scalar of ``values``, parameter), graph kept."""
        out = []
        for v in torch.cat([t.reshape(-1) for t in values]):
            out += [torch.autograd.grad(v, p, retain_graph=True, create_graph=True)[0]
                    for p in self._model.parameters() if p.requires_grad]
        return out

    def _update_gradients_and_hessian(self, loss, current_batch_size):
        grads = self._derivatives([loss[None]])
        hessian = torch.cat([t.reshape(-1) for t in self._derivatives(grads)]).reshape(self._final_hessian.shape)
        hessian = 0.5 * hessian + 0.5 * hessian.T
        share = current_batch_size / self._index_generator.n_samples
        self._n_samples_done += current_batch_size
        self._final_hessian += hessian.detach().cpu().numpy() * share
        self._final_gradients = [acc + g.detach().cpu().numpy() * share for acc, g in zip(self._final_gradients, grads)]

    def _local_train(self, train_dataset):
        penalty = sum(self._l2_coeff * torch.sum(p ** 2) / 2 for p in self._model.parameters())
        for xb, yb in torch.utils.data.DataLoader(train_dataset, batch_sampler=self._index_generator):
            xb, yb = xb.to(self._device), yb.to(self._device)
            self._update_gradients_and_hessian(self._criterion(self._model(xb), yb) + penalty, len(xb))

    @remote_data
    def train(self, data_from_opener, shared_state=None):
        ds = self._dataset(data_from_opener, is_inference=False)
        if shared_state is None:
            self._index_generator = self._instantiate_index_generator(len(ds))
        else:
            assert self._index_generator.n_samples is not None
            w.add_into(self._model, [torch.from_numpy(a).to(self._device) for a in shared_state.parameters_update],
                       self._with_batch_norm_parameters)
        self._index_generator.reset_counter()
        self._model.train()
        self._final_gradients, self._final_hessian, self._n_samples_done = self._initialize_gradients_and_hessian()
        self._local_train(ds)
        assert self._index_generator.n_samples == self._n_samples_done
        eigenvalues = np.linalg.eig(self._final_hessian)[0].real
        if not (eigenvalues >= 0).all():
            raise NegativeHessianMatrixError(f"negative eigenvalue: {eigenvalues.tolist()}, l2_coeff {self._l2_coeff}")
        self._index_generator.check_num_updates()
        return NewtonRaphsonSharedState(n_samples=self._index_generator.n_samples, hessian=self._final_hessian,
                                        gradients=self._final_gradients)
