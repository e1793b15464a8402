"""What the shipped Detector weights report under evaluate_detection on synthetic clips (a record for DESIGN.md section 4r, not a test):
    python tests/diag_detection_record.py [--out FILE]
tests/golden/detector_best_unprefixed.npz against an untrained seeded Generator(16) on four batches of 16 synthetic one-second clips,
undistorted and under white noise at 20 and 10 dB, with both scores and both decoders."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import awm_amd as awm                                                 # noqa: E402
from oracle import wm_oracle as O                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "diag_detection_record.py runs the models on the GPU"
    dev = torch.device("cuda:0")
    ck = np.load(os.path.join(ROOT, "tests", "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    G.to(dev); D.to(dev)
    batches = [O.synthetic_clips(16, seed=100 + i, T=16000) for i in range(4)]
    messages = [torch.randint(0, 2 ** 16, (16,), generator=torch.Generator().manual_seed(200 + i)) for i in range(4)]
    atk = {"noise 20 dB": awm.Distortion(gain_db=0, snr_db=20), "noise 10 dB": awm.Distortion(gain_db=0, snr_db=10)}
    lines = []
    for score, decode in (("prob", "vote"), ("vote", "llr")):
        for m in atk.values():
            m.reset(0)
        res = awm.evaluate_detection(G, D, batches, atk, device=dev, messages=messages, fpr_targets=(0.01, 0.1), score=score, decode=decode)
        for name, row in res.items():
            short = {k: (dict(v) if hasattr(v, "items") else v) for k, v in row.items() if k not in ("scores", "curve")}
            lines.append(f"score={score} decode={decode} {name}: {short!r}")
            mk, cl = row["scores"]["marked"], row["scores"]["clean"]
            lines.append(f"    marked scores min/median/max {np.min(mk):.4f} {np.median(mk):.4f} {np.max(mk):.4f}"
                         f"  clean {np.min(cl):.4f} {np.median(cl):.4f} {np.max(cl):.4f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
