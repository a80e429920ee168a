"""OneTransEvaluator — the offline evaluation of the reference (``practice/evaluate.py:22-129``).

The metrics are the trainer's running ones (``metrics.StreamingMetrics``): every batch adds to device state
with one launch, and the state is read once after the last batch.  The reference's plots, its placeholder
feature-importance numbers and its simulated A/B test are not part of the build.
"""

from __future__ import annotations

import json
import time
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch

from .config import OneTransConfig
from .metrics import GroupedAUC, StreamingMetrics
from .model import OneTransModel
from .trainer import _seq_inputs, _to_dev, stack_labels, stack_weights


class OneTransEvaluator:
    """evaluate.py:22-129 surface: ``evaluate_offline`` over an iterable of (non_seq, seq, labels) batches."""

    def __init__(self, model: OneTransModel, config: OneTransConfig, num_thresholds: int = 200,
                 group_feature: Optional[str] = None):
        """``group_feature`` (for example ``'user_id'``): ``evaluate_offline`` also reports the paper's user-level
        AUC of every binary task, ``{t}_uauc`` / ``_uauc_macro`` / ``_uauc_users`` / ``_uauc_impressions``
        (metrics.GroupedAUC), grouped by ``non_seq[group_feature]``."""
        self.model = model
        self.config = config
        self.device = model.flat.device
        # config.weighted_loss: the batches' weight keys (trainer.stack_weights) weigh every metric
        self.weighted = bool(getattr(config, 'weighted_loss', False))
        self.metrics = StreamingMetrics(config.tasks, self.device, num_thresholds, weighted=self.weighted)
        self.group_feature = group_feature
        self.grouped = GroupedAUC(config.tasks, self.device) if group_feature is not None else None

    @torch.no_grad()
    def evaluate_offline(self, batches) -> Dict:
        """``training=False`` forwards over ``batches``; returns the reference's metrics (evaluate.py:39-56:
        AUC, accuracy, precision, recall, F1 and logloss for the binary tasks, MSE and MAE for the others)
        plus ``performance`` (evaluate.py:118-123): total samples, samples per second and the mean time per
        batch and per sample.

        The whole pass is timed between two device synchronisations and divided by the number of batches.
        The reference wraps each model call in ``time.time()``; on an asynchronous device that measures only
        how long the launches take to issue, not how long the batch takes to compute."""
        dev = self.device
        self.metrics.reset_states()
        if self.grouped is not None:
            self.grouped.reset_states()
        total_samples, nbatches = 0, 0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for non_seq, seq, labels in batches:
            y = labels if isinstance(labels, torch.Tensor) else stack_labels(labels, self.config.tasks, dev)
            w = stack_weights(labels, self.config, dev) if self.weighted else None
            if w is not None and self.grouped is not None:
                raise NotImplementedError('weighted_loss with group_feature: the grouped AUC (UAUC) carries no sample '
                                          'weights; drop the weight keys or the group feature')
            probs = self.model.forward_probs(_to_dev(non_seq, dev), _seq_inputs(self.model, seq, dev), training=False)
            if self.weighted:
                self.metrics.update(y, probs, weights=w)
            else:
                self.metrics.update(y, probs)
            if self.grouped is not None:
                if self.group_feature not in non_seq:
                    raise KeyError(f'OneTransEvaluator(group_feature={self.group_feature!r}): the batch has no '
                                   f'non-sequence feature of that name (it has {sorted(non_seq)})')
                ids = torch.as_tensor(non_seq[self.group_feature]).reshape(-1).to(dev, torch.int64)
                self.grouped.update(ids, y, probs)
            total_samples += int(y.shape[1])
            nbatches += 1
        torch.cuda.synchronize(dev)
        elapsed = time.perf_counter() - t0
        results = self.metrics.result(extended=True)
        if self.grouped is not None:
            results.update(self.grouped.result())
        results['performance'] = {
            'total_samples': total_samples,
            'avg_inference_time_per_batch': elapsed / nbatches if nbatches else 0.0,
            'throughput_samples_per_second': total_samples / elapsed if elapsed > 0 else 0.0,
            'avg_inference_time_per_sample': elapsed / total_samples if total_samples else 0.0,
        }
        return results


def load_model_for_evaluation(model_path: str, device=None) -> Tuple[OneTransModel, OneTransConfig]:
    """evaluate.py's loader: ``config.json`` + ``model_weights.npz`` of a checkpoint directory written by
    ``OneTransTrainer.save_model``."""
    path = Path(model_path)
    with open(path / 'config.json') as f:
        config = OneTransConfig.from_dict(json.load(f))
    model = OneTransModel(config, device=device)
    model.load_weights(str(path / 'model_weights.npz'))
    return model, config
