"""Drop-in `utils` package exporting RMSNorm (reference: utils/__init__.py, `from utils import RMSNorm`
at meant/meant.py:13) and f1_metrics (`from utils import f1_metrics` at in_loop_train.py:30, test_run.py:27); balanced_class_weights, the one-line
alternative to the reference's offline smote.py, sits beside them."""
from meant_amd.modules import RMSNorm  # noqa: F401
from meant_amd.metrics import f1_metrics  # noqa: F401
from meant_amd.train import balanced_class_weights  # noqa: F401
