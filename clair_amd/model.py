"""Drop-in for ``clair.model.Clair`` on MI355X: the inference surface and the training members.

Mirrors the members call_var / evaluate / train use on the reference class
(/root/reference/clair/model.py):

  Clair(**kwargs)              :58-192   constructor (graph build + session there; engine handle here)
  .init()                      :807-813  marks the model initialised; fresh weights are drawn only if it trains or predicts with nothing restored
  .restore_parameters(prefix)  :1016-1020  load a weight container / checkpoint prefix
  .predict(batchX)             :946-966  -> [gt21 [n,21], genotype [n,3], len1 [n,33], len2 [n,33]]
                                          float32; also stored in ``self.prediction``
  .prediction                  :964
  .close() / __del__           :872-876, 1149-1152
  .train(batchX, batchY)       :913-944  one optimizer step on the batch -> training_loss_on_one_batch
  .lr_train(batchX, batchY)    :878-911  train() that keeps the training pass's prediction and its accuracy (docs/train_clr.md)
  .clr(step, step_size, max_lr, mode)  :1086-1103  the cyclical learning rate, advanced once per batch
  .validate(batchX, batchY)    :968-1008 the loss members of one batch
  .save_parameters(prefix)     :1010-1014 a checkpoint under the reference's variable names
  .set_learning_rate / decay_learning_rate / set_l2_regularization_lambda / decay_l2_regularization_lambda / set_task_loss_weights

Training runs in float32 HIP kernels behind the trainer handle of the C ABI (clair_train_*, docs/train.md); the trainer is made on first use
and the engine is handed the trained weights when predict / evaluate next need them.

The forward pass itself runs in hand-written HIP kernels behind the C ABI of
include/clair_amd.h (clair_amd/csrc); there is no CPU or framework fallback.
"""
import numpy as np

from clair_amd import _capi, param, weights


def training_defaults():
    """The training entries of the reference's params dictionary (clair/model.py:61-105)."""
    return dict(
        task_loss_weights=[1, 1, 1, 1, 1],                   # gt21, genotype, indel length 1, indel length 2, l2
        output_gt21_entropy_weights=[1] * 21,
        output_genotype_entropy_weights=[1] * 3,
        output_indel_length_entropy_weights_1=[1] * 33,
        output_indel_length_entropy_weights_2=[1] * 33,
        L4_dropout_rate=0.5, L5_1_dropout_rate=0.2, L5_2_dropout_rate=0.2, L5_3_dropout_rate=0.2, L5_4_dropout_rate=0.2,
        LSTM2_dropout_rate=0.5,
        initial_learning_rate=param.initialLearningRate,
        learning_rate_decay=param.learningRateDecay,
        l2_regularization_lambda=param.l2RegularizationLambda,
        l2_regularization_lambda_decay_rate=param.l2RegularizationLambdaDecay,
        optimizer_name=param.default_optimizer,
        loss_function=param.default_loss_function,
    )


def accuracy_counts(probabilities, labels):
    """The learning-rate finder's accuracy rule (clair/learning_rate_finder.py:21-73) as counts: probabilities [n,90] packed as the outputs
    are, labels [n,4] true indices -> int64 [4], the rows whose gt21 arg-max is the label, whose genotype arg-max is, and -- the two
    indel-length heads taken as sorted pairs -- whose smaller arg-max is the smaller label and whose larger is the larger.  np.argmax: the
    lowest index among equal values.  The NumPy twin of clair_train_accuracy (csrc/train_accuracy.hip.h)."""
    p, y = np.asarray(probabilities), np.asarray(labels).astype(np.int64)
    if p.ndim != 2 or p.shape[1] != 90 or y.shape != (p.shape[0], 4):
        raise ValueError("probabilities [n,90] and labels [n,4] expected, got %r and %r" % (p.shape, y.shape))
    top = np.stack([np.argmax(p[:, a:b], axis=1) for a, b in ((0, 21), (21, 24), (24, 57), (57, 90))], axis=1).reshape(-1, 4)
    hits = [top[:, 0] == y[:, 0], top[:, 1] == y[:, 1],
            top[:, 2:].min(axis=1) == y[:, 2:].min(axis=1), top[:, 2:].max(axis=1) == y[:, 2:].max(axis=1)]
    return np.array([int(h.sum()) for h in hits], dtype=np.int64)


def accuracy_from_counts(tp, n):
    """The reference's arithmetic in its order (clair/learning_rate_finder.py:68-72): the mean of the four heads' hit rates over n rows."""
    n = n + 0.0
    return (tp[0] / n + tp[1] / n + tp[2] / n + tp[3] / n) / 4


class Clair(object):
    """MI355X engine and trainer behind the reference's ``Clair`` interface."""

    def __init__(self, **kwargs):
        self.device = int(kwargs.pop("device", 0))
        self.max_batch = int(kwargs.pop("max_batch", max(param.predictBatchSize, 1024)))
        self.n_slots = int(kwargs.pop("n_slots", 2))
        self.micro_batch = int(kwargs.pop("micro_batch", param.trainMicroBatchSize))
        self.seed = int(kwargs.pop("seed", 0) or 0)
        params = training_defaults()
        # the reference reports unsupported kwargs instead of failing (clair/model.py:112-116)
        for key, value in kwargs.items():
            if key in params:
                params[key] = value
            else:
                print("Info: the parameter %s, with value %s is not supported" % (key, value))
        self.task_loss_weights = np.array(params["task_loss_weights"], dtype=float)
        self.output_gt21_entropy_weights = np.array(params["output_gt21_entropy_weights"], dtype=float)
        self.output_genotype_entropy_weights = np.array(params["output_genotype_entropy_weights"], dtype=float)
        self.output_indel_length_entropy_weights_1 = np.array(params["output_indel_length_entropy_weights_1"], dtype=float)
        self.output_indel_length_entropy_weights_2 = np.array(params["output_indel_length_entropy_weights_2"], dtype=float)
        for key in ("L4_dropout_rate", "L5_1_dropout_rate", "L5_2_dropout_rate", "L5_3_dropout_rate", "L5_4_dropout_rate", "LSTM2_dropout_rate"):
            setattr(self, key, params[key])
        self.learning_rate_value = params["initial_learning_rate"]
        self.learning_rate_decay_rate = params["learning_rate_decay"]
        self.l2_regularization_lambda_value = params["l2_regularization_lambda"]
        self.l2_regularization_lambda_decay_rate = params["l2_regularization_lambda_decay_rate"]
        self.optimizer_name = params["optimizer_name"]
        self.loss_function = params["loss_function"]
        if self.optimizer_name not in _capi.Trainer.OPTIMIZERS or self.loss_function not in _capi.Trainer.LOSSES:
            raise ValueError("optimizer_name is one of %r and loss_function one of %r" % (_capi.Trainer.OPTIMIZERS, _capi.Trainer.LOSSES))
        self._trainer = None
        self._weights = None                # the host copy the trainer is started from (init / restore_parameters / set_parameters)
        self._initialised = False           # init() was called: a model that restores nothing may draw fresh weights when it first needs some
        self._host_stale = False            # the trainer has stepped since its weights were last downloaded
        self._engine_stale = False          # ... since the engine was last handed weights
        self._l2 = None                     # sum w^2 / 2 over the kernels of the current weights, once asked for
        self.input_shape = (2 * param.flankingBaseNum + 1, param.matrixRow, param.matrixNum)
        self.output_gt21_shape = 21
        self.output_genotype_shape = 3
        self.output_indel_length_shape_1 = 33
        self.output_indel_length_shape_2 = 33
        self.prediction = None
        self.layers = []
        self._engine = _capi.Engine(self.device, self.max_batch, self.n_slots)
        self._weights_loaded = False

    # -- reference interface ---------------------------------------------------------------
    def init(self):
        """clair/model.py:807-813 runs the TF initialiser.  Here nothing is drawn yet: every caller that restores a checkpoint next pays
        nothing.  A model that restores nothing draws its weights (weights.synthetic_weights: the reference's initialisers, seeded by the
        `seed` keyword) when train / validate / predict / get_parameters first need them."""
        self._initialised = True

    def _need_weights(self):
        if self._weights is None and self._initialised:
            self.set_parameters(weights.synthetic_weights(seed=20250928 + self.seed))

    def restore_parameters(self, file_name):
        """clair/model.py:1016-1020.  ``file_name`` is a checkpoint prefix (or an .npz container)."""
        self.set_parameters(weights.load_weights(file_name))

    def set_parameters(self, w):
        """Load weights from a dict of arrays keyed as clair_amd.weights.TENSOR_TABLE."""
        self._engine.load_weights(w)
        self._weights_loaded = True
        self._weights = w
        self._host_stale = self._engine_stale = False
        self._l2 = None
        if self._trainer is not None:       # the optimizer state stays, as a tf.train.Saver restore of the trainable variables alone would leave it
            self._trainer.set_tensors(w)

    # -- training (clair/model.py:913-944, 968-1014) ---------------------------------------------------------
    @property
    def trainer(self):
        if self._trainer is None:
            self._need_weights()
            if self._weights is None:
                raise _capi.EngineError("no weights to train: call init() or restore_parameters() first")
            self._trainer = _capi.Trainer(self.device, self.micro_batch, self.optimizer_name, self.loss_function)
            self._trainer.set_tensors(self._weights)
        return self._trainer

    def _configure_trainer(self):
        t = self.trainer
        t.config(self.task_loss_weights,
                 np.concatenate([self.output_gt21_entropy_weights, self.output_genotype_entropy_weights, self.output_indel_length_entropy_weights_1,
                                 self.output_indel_length_entropy_weights_2]),
                 [self.LSTM2_dropout_rate, self.L4_dropout_rate, self.L5_1_dropout_rate, self.L5_2_dropout_rate, self.L5_3_dropout_rate, self.L5_4_dropout_rate],
                 self.seed)
        return t

    @staticmethod
    def label_indices(batchY):
        """[n,90] one-hot rows as the reference passes them, or uint8 [n,4] true indices -> uint8 [n,4]"""
        y = np.asarray(batchY)
        if y.ndim == 2 and y.shape[1] == 90:
            return np.stack([np.argmax(y[:, a:b], axis=1) for a, b in ((0, 21), (21, 24), (24, 57), (57, 90))], axis=1).astype(np.uint8)
        if y.ndim == 2 and y.shape[1] == 4:
            return np.ascontiguousarray(y, dtype=np.uint8)
        raise ValueError("batchY must be [n,90] one-hot rows or [n,4] indices, got shape %r" % (y.shape,))

    def _accumulate(self, batchX, batchY, training, accuracy=False):
        """-> (trainer, losses [4], probabilities of each micro-batch -- kept for validation and when `accuracy` is asked for --, tp int64 [4]:
        the accuracy counts of the micro-batches added up on the way, zeros unless asked for)"""
        t = self._configure_trainer()
        x, lab = np.asarray(batchX), self.label_indices(batchY)
        losses, probabilities, tp = np.zeros(4), [], np.zeros(4, dtype=np.int64)
        for first in range(0, x.shape[0], self.micro_batch):
            losses += t.accumulate(x[first:first + self.micro_batch], lab[first:first + self.micro_batch], first_row=first, training=training)
            if accuracy:
                tp += t.accuracy()
            if accuracy or not training:
                probabilities.append(t.probabilities())
        return t, losses, probabilities, tp

    def train(self, batchX, batchY):
        """clair/model.py:913-944: one optimizer step on the batch, cut into micro-batches whose gradients are summed.
        training_loss_on_one_batch is the weighted total with lambda * L2 (:697-709)."""
        t = self.trainer
        t.zero_grad()
        t, losses, _, _ = self._accumulate(batchX, batchY, True)
        return self._step(t, losses), None

    def lr_train(self, batchX, batchY):
        """clair/model.py:878-911: train() that also keeps what the training forward pass (dropout on) predicted, for the learning-rate finder.
        `prediction`: the four heads' probabilities, shaped as validation_prediction; `training_tp`: int64 [4], the rows each head gets right
        under the finder's rule, counted on the device per micro-batch (clair_train_accuracy) and added up; `training_accuracy`: the
        accuracy of those counts (accuracy_from_counts).  -> (prediction, training_loss_on_one_batch, None)"""
        t = self.trainer
        t.zero_grad()
        t, losses, probabilities, tp = self._accumulate(batchX, batchY, True, accuracy=True)
        self.prediction = _capi.split_outputs(np.concatenate(probabilities, axis=0))
        self.training_tp = tp
        self.training_accuracy = accuracy_from_counts(tp, len(self.prediction[0]))
        return self.prediction, self._step(t, losses), None

    def _step(self, t, losses):
        """The optimizer step after the micro-batches of a batch -> training_loss_on_one_batch"""
        l2, norm = t.step(self.learning_rate_value, self.l2_regularization_lambda_value)
        self._host_stale = self._engine_stale = True
        self._l2 = None
        self.gradient_norm_on_one_batch = norm
        self.training_loss_on_one_batch = float(np.dot(self.task_loss_weights[:4], losses) + self.task_loss_weights[4] * l2 * self.l2_regularization_lambda_value)
        self.training_summary_on_one_batch = None
        return self.training_loss_on_one_batch

    def validate(self, batchX, batchY):
        """clair/model.py:968-1008: the forward pass without dropout; lambda is fed as 0 there, so the total has no L2 part, and l2_loss is
        the L2 sum times param.l2RegularizationLambda."""
        t, losses, probabilities, _ = self._accumulate(batchX, batchY, False)
        self.validation_prediction = _capi.split_outputs(np.concatenate(probabilities, axis=0))
        self.validation_loss_on_one_batch = float(np.dot(self.task_loss_weights[:4], losses))
        self.gt21_loss, self.genotype_loss, self.indel_length_loss_1, self.indel_length_loss_2 = (float(v) for v in losses)
        self.indel_length_loss = self.indel_length_loss_1 + self.indel_length_loss_2
        if self._l2 is None:                # once per set of weights, not per validation batch
            self._l2 = float(sum(np.sum(np.asarray(v, dtype=np.float64) ** 2) / 2 for k, v in self.get_parameters().items() if not k.endswith("_bias")))
        self.l2_loss = self._l2 * param.l2RegularizationLambda
        return self.validation_loss_on_one_batch

    def get_parameters(self):
        """The current weights as a dict keyed as clair_amd.weights.TENSOR_TABLE (downloaded from the trainer once after it stepped)."""
        self._need_weights()
        if self._host_stale:
            self._weights = self._trainer.get_tensors()
            self._host_stale = False
        return self._weights

    def _sync_engine(self):
        """Hand the engine the trained weights if the trainer has stepped since it last got some."""
        if self._engine_stale:
            self._engine.load_weights(self.get_parameters())
            self._engine_stale = False

    def save_parameters(self, file_name):
        """clair/model.py:1010-1014: a TF-bundle checkpoint (prefix.index / .data-00000-of-00001) under the reference's variable names."""
        from clair_amd import tf_bundle
        tf_bundle.export_checkpoint(file_name, self.get_parameters())

    def set_task_loss_weights(self, task_loss_weights=[1, 1, 1, 1, 1]):
        self.task_loss_weights = np.array(task_loss_weights, dtype=float)

    def set_learning_rate(self, learning_rate):
        self.learning_rate_value = learning_rate
        return self.learning_rate_value

    def decay_learning_rate(self):
        self.learning_rate_value = self.learning_rate_value * self.learning_rate_decay_rate
        return self.learning_rate_value

    def clr(self, global_step, step_size, max_lr, mode="tri"):
        """clair/model.py:1086-1103, the cyclical learning rate: one call per batch.  The rate climbs from param.clr_min_lr to max_lr over
        step_size calls and back over the next step_size; the call after that (the one whose 1 + step / (2 step_size) passes 2) starts the
        next cycle at the floor, with max_lr halved (tri2), times param.clrGamma (exp) or as it was (tri).
        -> (learning_rate_value, global_step, max_lr): the caller carries the last two into its next call.  The arithmetic is the
        reference's, operation by operation, so the rates are equal as float64 values."""
        global_step += 1
        if 1 + global_step / (2 * step_size) > 2:
            global_step = 0
            max_lr = max_lr / 2 if mode == "tri2" else max_lr * param.clrGamma ** 1 if mode == "exp" else max_lr
        x = global_step / step_size
        self.learning_rate_value = param.clr_min_lr + (max_lr - param.clr_min_lr) * np.maximum(0, x if x <= 1 else 2 - x)
        return self.learning_rate_value, global_step, max_lr

    def set_l2_regularization_lambda(self, l2_regularization_lambda):
        self.l2_regularization_lambda_value = l2_regularization_lambda
        return self.l2_regularization_lambda_value

    def decay_l2_regularization_lambda(self):
        self.l2_regularization_lambda_value = self.l2_regularization_lambda_value * self.l2_regularization_lambda_decay_rate
        return self.l2_regularization_lambda_value

    def restore_ensemble(self, file_names):
        """restore_parameters for an ensemble: the reference makes one Clair and one call_var run per checkpoint and averages their
        --output_for_ensemble rows (clair/post_processing/ensemble.py:10-75); here one engine holds them all and submit_ensemble runs
        them over each batch.  The first prefix is the model predict / submit go on using alone."""
        self.set_ensemble([weights.load_weights(f) for f in file_names])

    def set_ensemble(self, list_of_weights):
        self._engine.load_ensemble(list_of_weights)
        self._weights_loaded = True

    @property
    def n_models(self):
        return self._engine.n_models

    def predict(self, batchX):
        """clair/model.py:946-966: list of four float32 arrays; kept in ``self.prediction``."""
        self._need_weights()
        self._sync_engine()
        x = np.asarray(batchX)
        n = x.shape[0]
        if n <= self.max_batch:
            prediction = self._engine.predict(x)
        else:  # larger than one engine batch: pipeline max_batch pieces over the slots
            prediction = self._predict_pieces(x)
        self.prediction = prediction
        return prediction

    def close(self):
        if getattr(self, "_trainer", None) is not None:
            self._trainer.close()
            self._trainer = None
        if getattr(self, "_engine", None) is not None:
            self._engine.close()
            self._engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_summary_file_writer(self, logs_path):
        """Dead path in the reference too (clair/model.py:1053-1062 returns None)."""
        return None

    # -- pipelined helpers (used by clair_amd.call_var) ----------------------------------------
    def submit(self, slot, batchX):
        self._engine.submit(slot, batchX)

    def submit_counts(self, slot, counts):
        """submit() for raw pileup counts [n,33,8,4] int16 (before clair/utils.py:96-98): the subtraction and the conversion
        run on the device, the host link carries half the bytes.  Same outputs as submit() on the float32 tensor."""
        self._engine.submit_counts(slot, counts)

    def submit_calls(self, slot, batch, centre, counts=False, with_probabilities=False):
        """Forward pass + decode on the device (include/clair_amd.h: clair_submit_ex): wait(slot) returns the call records of
        include/clair_call.h -- or (records, probabilities) -- instead of the probabilities."""
        self._engine.submit_calls(slot, batch, centre, counts=counts, with_probabilities=with_probabilities)

    def submit_ensemble(self, slot, batch, centre=None, counts=False, with_probabilities=False):
        """submit_calls over every checkpoint of restore_ensemble, averaged on the device (include/clair_amd.h: clair_submit_ensemble);
        centre=None: no decode, wait(slot) returns the averaged probabilities."""
        self._engine.submit_ensemble(slot, batch, centre, counts=counts, with_probabilities=with_probabilities)

    def site_table(self):
        """A site table of the engine for ensemble calling across BAMs (include/clair_amd.h: clair_sites_*; docs/ensemble.md)."""
        return self._engine.site_table()

    def submit_sites(self, slot, table, first, batch, centre, seq, counts=False):
        """Every checkpoint over the batch, folded into `table` as candidates [first, first + n) of its current source."""
        self._engine.submit_sites(slot, table, first, batch, centre, seq, counts=counts)

    def submit_site_calls(self, slot, table, first, n, with_calls=True, with_probabilities=False):
        """The decode of entries [first, first + n) of the table's output list; wait(slot) returns what it returns after submit_ensemble."""
        self._engine.submit_site_calls(slot, table, first, n, with_calls=with_calls, with_probabilities=with_probabilities)

    def pinned_buffer(self, nbytes):
        """Page-locked host memory of the engine (include/clair_amd.h: clair_pinned_alloc) as a uint8 array."""
        return self._engine.pinned_buffer(nbytes)

    def wait(self, slot):
        return self._engine.wait(slot)

    def _predict_pieces(self, x):
        pieces, inflight = [], []
        mb, ns = self.max_batch, self.n_slots
        for k, start in enumerate(range(0, x.shape[0], mb)):
            slot = k % ns
            if len(inflight) == ns:
                pieces.append(self._engine.wait(inflight.pop(0)))
            self._engine.submit(slot, x[start:start + mb])
            inflight.append(slot)
        while inflight:
            pieces.append(self._engine.wait(inflight.pop(0)))
        return [np.concatenate([p[i] for p in pieces], axis=0) for i in range(4)]

    @property
    def engine(self):
        self._sync_engine()
        return self._engine
