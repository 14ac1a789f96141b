"""From a KITTI directory to the AP table: the use DGDE/engine/inference.py:19-125 makes of the model, the result writer and
the evaluator.  One image per model call, as the reference runs its evaluation (TEST.IMS_PER_BATCH = 1); every image's
`PostProcessor` rows go to `<output_folder>/data/<id>.txt`, then the files are read back and evaluated against `label_2`
on the device.  No visualisation and no `gen_data` branch."""
import logging
import os

import torch

from dcd_amd.eval import kitti_annos, kitti_ap


def inference(model, files, pipeline, output_folder, metrics=("R40",)):
    """model: a `KeypointDetector`; files: a `KittiFiles`; pipeline: a `DeviceInputPipeline(is_train=False)`.
    Returns {metric: the dict of `kitti_ap.official_eval`}."""
    if pipeline.is_train:
        raise ValueError("inference needs a DeviceInputPipeline(is_train=False): evaluation never flips")
    logger = logging.getLogger("dcd_amd.inference")
    predict_folder = os.path.join(output_folder, "data")
    os.makedirs(predict_folder, exist_ok=True)
    ids = [files.img_id(i) for i in range(len(files))]
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i, img_id in enumerate(ids):
                images, targets = pipeline([files.frame(i)], [files.sample(i)], img_ids=[img_id])
                rows = model(images, targets)[0]
                kitti_annos.write_detections(rows, os.path.join(predict_folder, img_id + ".txt"))
    finally:
        model.train(was_training)
    dt_annos = kitti_annos.read_annos(predict_folder, ids)
    gt_annos = kitti_annos.read_annos(os.path.join(files.root, "label_2"), ids)
    results = {}
    for metric in metrics:
        text, results[metric] = kitti_ap.official_eval(gt_annos, dt_annos, list(files.classes), metric=metric,
                                                       device=pipeline.device)
        logger.info("%s\n%s", metric, text)
    return results
