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

    def _accumulate(self, batchX, batchY, training):
        t = self._configure_trainer()
        x, lab = np.asarray(batchX), self.label_indices(batchY)
        losses, probabilities = np.zeros(4), []
        for first in range(0, x.shape[0], self.micro_batch):
            losses += t.accumulate(x[first:first + self.micro_batch], lab[first:first + self.micro_batch], first_row=first, training=training)
            if not training:
                probabilities.append(t.probabilities())
        return t, losses, probabilities

    def train(self, batchX, batchY):
        """clair/model.py:913-944: one optimizer step on the batch, cut into micro-batches whose gradients are summed.
        training_loss_on_one_batch is the weighted total with lambda * L2 (:697-709)."""
        t = self.trainer
        t.zero_grad()
        t, losses, _ = self._accumulate(batchX, batchY, True)
        l2, norm = t.step(self.learning_rate_value, self.l2_regularization_lambda_value)
        self._host_stale = self._engine_stale = True
        self._l2 = None
        self.gradient_norm_on_one_batch = norm
        self.training_loss_on_one_batch = float(np.dot(self.task_loss_weights[:4], losses) + self.task_loss_weights[4] * l2 * self.l2_regularization_lambda_value)
        self.training_summary_on_one_batch = None
        return self.training_loss_on_one_batch, None

    def validate(self, batchX, batchY):
        """clair/model.py:968-1008: the forward pass without dropout; lambda is fed as 0 there, so the total has no L2 part, and l2_loss is
        the L2 sum times param.l2RegularizationLambda."""
        t, losses, probabilities = self._accumulate(batchX, batchY, False)
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
