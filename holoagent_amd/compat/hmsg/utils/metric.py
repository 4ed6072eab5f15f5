"""fsr_vln/memory/hmsg/utils/metric.py under its own import path (holoagent_amd/semseg.py)."""
from holoagent_amd.semseg import (EvalSegErr, frequency_weighted_iou, mean_accuracy, mean_iou, per_class_iou,  # noqa: F401
                                  pixel_accuracy)
