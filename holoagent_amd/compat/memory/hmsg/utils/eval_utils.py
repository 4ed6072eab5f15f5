"""fsr_vln/memory/hmsg/utils/eval_utils.py under its own import path: the semantic segmentation evaluation (holoagent_amd/semseg.py)."""
from holoagent_amd.semseg import (Tree_interpolation, knn_interpolation, load_feature_map, sim_2_label,  # noqa: F401
                                  text_prompt)
