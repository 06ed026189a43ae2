"""The whole training step of ``DiffusionModel`` on the MI355X (BASELINE configs[4]).

``TrainModel`` runs the reference's ``DiffusionModel.forward`` in train mode (model.py:133-199) and the backward pass its
``loss.backward()`` would run (train.py:55-60), as a chain of hand-written fp32 HIP operations (include/dhw_train.h
``dhw_op_*``: one strided exact-f32 MFMA GEMM for every Linear / Conv1d / attention product in all three directions, plus
FiLM, LayerNorm, softmax, resampling, embedding and activation kernels).  torch supplies device memory and streams only:
no torch operator touches an activation or a gradient.  The op order mirrors the reference module by module so that the
recorded tape, replayed in reverse, accumulates exactly autograd's gradients; ``tests/test_gpu_train.py`` pins every one
of the 323 parameter gradients against a fixture the imported reference generated (tests/golden/model_grad.npz).

Parameters keep the reference's ``state_dict`` names and torch layouts, so a reference checkpoint loads unchanged and a
trained one can be handed straight to ``dhg_amd.DiffusionModel`` for sampling.

One module per concern, each importing only the ones before it: ``tape`` (Var, Tape; DHW_TRAIN_FUSE_DSILU), ``net`` (TrainModel;
DHW_TRAIN_FILM_RIDER), ``data`` (ResidentData), ``step`` (train_step, GraphedTrainStep; DHW_TRAIN_BUCKETS), ``state`` (save_train_state,
load_train_state), ``evaluate`` (EvalStep), ``loop`` (fit).  Each
environment switch is read once, at import, by the module named with it.
"""
from .tape import FUSE_DSILU, Tape, Var, _ViewVar  # noqa: F401
from .net import FILM_RIDER, N_BUCKETS, TrainModel, grad_bucket, positional_encoding  # noqa: F401
from .data import ResidentData, group_tables  # noqa: F401
from .step import GRAD_BUCKETS, GraphedTrainStep, train_step  # noqa: F401
from .state import load_train_state, read_train_state, save_train_state  # noqa: F401
from .evaluate import EvalStep  # noqa: F401
from .loop import fit, read_train_config  # noqa: F401
