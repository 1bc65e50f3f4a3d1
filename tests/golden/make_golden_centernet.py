#!/usr/bin/env python3
"""Mint the edge-shape CenterNet fixtures by running the REFERENCE's src/centernet_target.py and src/fusion_detection.py
(build container only; imported through make_golden.import_reference(), never copied).

    targets_<case>.npz          prepare_centernet_targets on every tests.golden.cases.CN_TARGET_CASES entry
    decode_{ct,fd}_<case>.npz   decode_centernet_predictions on the CN_DECODE_CASES entries marked `fixture`; they must be free
                                of ties at both cuts (asserted), since torch.topk leaves the order of equal scores open

Inputs come from tests/golden/cases (counter-based generator); the fixtures hold outputs only, each under 64 KiB (asserted;
the many-object cases draw their boxes from a small lattice of values so that all 12 tensors fit)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import centernet_ref as R                                       # noqa: E402
from tests.golden import cases                                             # noqa: E402
from tests.golden.make_golden import import_reference, save                # noqa: E402

LIMIT = 64 * 1024


def size_of(name):
    return os.path.getsize(os.path.join(HERE, name + ".npz"))


@torch.no_grad()
def main():
    torch.set_num_threads(1)
    _, _, ct, fd = import_reference()
    for c in cases.CN_TARGET_CASES:
        boxes, labels = cases.cn_target_inputs(c)
        t = ct.prepare_centernet_targets({"gt_boxes": boxes, "gt_labels": labels}, torch.device("cpu"), **cases.cn_target_kwargs(c))
        name = "targets_" + c["name"]
        save(name, **t)
        assert size_of(name) <= LIMIT, (name, size_of(name))
    for c in cases.CN_DECODE_CASES:
        if not c.get("fixture"):
            continue
        pred = cases.cn_decode_predictions(c)
        assert c["masked"] and R.tie_counts(pred["heatmap"], c["K"], True) == (0, 0), c["name"]
        thresh = R.case_thresh(c, R.topk_spec(pred["heatmap"], c["K"], True))
        for tag, fn in (("ct", ct.decode_centernet_predictions), ("fd", fd.decode_centernet_predictions)):
            dets = fn(pred, score_thresh=thresh, max_detections=c["K"])
            flat = {f"{k}_{b}": v for b, d in enumerate(dets) for k, v in d.items()}
            name = f"decode_{tag}_{c['name']}"
            save(name, **flat)
            assert size_of(name) <= LIMIT, (name, size_of(name))


if __name__ == "__main__":
    main()
