"""GMW (graph matching weighting) train step -- SURVEY.md section 8(f) rank 1: the direct consumer of the edge-constraint
depth solver.  Mirrors GMW/model/model.py, GMW/lib/optimal_transport.py and the step of GMW/main.py:447-466; inference.py is
the second stage itself: a detector's records -> refined result files -> KITTI AP (main.py:123-215, 524-548); data.py and
train.py train the model from the detector's generated records (main.py:231-341, 418-484)."""
from .model import GMW, pairwise_l2_dist                      # noqa: F401
from .optimal_transport import RegularisedTransport          # noqa: F401
from .step import compute_reg_loss, correspondence_loss, gmw_losses, gmw_train_step, gmw_val_step    # noqa: F401
from .inference import (RecordRefiner, evaluate, extract_features, load_infer_data, plan_packs, refine, refine_packed,    # noqa: F401
                        write_results, writer_fields)
from .data import ResidentRecords, epoch_order, load_train_data    # noqa: F401
from .train import train_gmw                                  # noqa: F401
