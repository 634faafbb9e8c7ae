"""Drop-in for the reference's top-level `metrics` module.

The reference's training drivers import the validation metrics by this module name (train.py:17, dist_train.py:
`from metrics import feature_metric, edge_error_metric`).  With this repository ahead of the reference checkout on
`sys.path` that line resolves here: `feature_metric` keeps its sums on the device (one launch per recorded batch, one
read-back per epoch; `graingraphnn_amd.metrics`) behind the reference's interface -- `record`, `epoch_summary`, `summary`,
and the attributes the drivers read afterwards (`metric_list`, `test_auc`, `plist`, `rlist`).  train.py itself is not edited.
"""
from graingraphnn_amd.metrics import edge_error_metric, feature_metric

__all__ = ["feature_metric", "edge_error_metric"]
