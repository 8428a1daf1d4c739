"""Tensor geometry and batch defaults (counterpart of /root/reference/shared/param.py:1-16).

Inference geometry first, then the training hyper-parameters of shared/param.py:4-37 that clair_amd.train and Clair.train read.
"""
REPO_NAME = "Clair"
NUM_THREADS = 12            # shared/param.py:3 (host-side threads; the GPU engine ignores it)
flankingBaseNum = 16        # shared/param.py:9
matrixRow = 8               # shared/param.py:10
matrixNum = 4               # shared/param.py:11
predictBatchSize = 1000     # shared/param.py:16
engineBatchSize = 4096      # candidates per forward pass when --batch_size is not given: results do not depend on it, and at the reference's 1 000 the
                            # host side of call_var (queues, ctypes calls, one NumPy view per batch) keeps the engine at half its rate
                            # (3.0-4.1 against 5.3-6.7 M candidates/s inside call_variants, profiles/r04_e2e_binary.txt)
# training (shared/param.py)
parameterOutputPlaceHolder = 6      # :4   digits of the epoch number in a checkpoint name
bloscBlockSize = 500                # :12  rows of one shuffling block
trainBatchSize = 10000              # :15
initialLearningRate = 1e-3          # :17
learningRateDecay = 0.1             # :18
maxLearningRateSwitch = 3           # :19
trainingDatasetPercentage = 0.9     # :20
l2RegularizationLambda = 0.005      # :23
l2RegularizationLambdaDecay = 1     # :24
default_optimizer = "Adam"          # :28  Adam / SGDM
default_loss_function = "FocalLoss"  # :29  CrossEntropy / FocalLoss
clr_max_lr = 3e-2                   # :32  train_clr: the rate a cycle rises to (before tri2 / exp decay it)
clr_min_lr = 1e-4                   # :33  the floor of every cyclical rate, the finder's sweep included
stepsizeConstant = 1                # :34  half a cycle, in epochs' worth of batches
clrGamma = 0.95                     # :35  exp mode: max_lr is multiplied by it after each cycle
momentum = 0.9                      # :36
maxEpoch = 30                       # :37
min_lr = 1e-6                       # :40  learning_rate_finder: only logged (the sweep starts from clr_min_lr)
max_lr = 1e-1                       # :41  learning_rate_finder: the top of the sweep
lr_finder_max_epoch = 1             # :42
RANDOM_SEED = None                  # :47
trainMicroBatchSize = 1024          # rows per forward + backward pass on the device (about 0.59 MB of workspace each, docs/train.md)
no_of_positions = 2 * flankingBaseNum + 1
input_tensor_size = no_of_positions * matrixRow * matrixNum  # 1056


def pipeline_slots():
    """Batches the callers keep in flight at the engine's host boundary (clair_submit* / clair_wait).  Three compute lanes fill the
    chip; twice as many slots keep every lane fed while its other batch is on the host link.  CLAIR_AMD_SLOTS
    overrides (1 and 2 select the fused layer-2 launch of one- and two-lane handles; up to 4 slots get a lane each -- the configuration of a
    caller whose batches are already in HBM -- and 4 slots fed from the host are the one bad choice: four lanes and the copy stream are five
    streams on four hardware queues)."""
    import os
    try:
        return max(1, min(64, int(os.environ.get("CLAIR_AMD_SLOTS", "6"))))
    except ValueError:
        return 6
