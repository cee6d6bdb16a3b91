"""Records tests/golden/metrics_parent_fit.npz: loss history and final weights of tests/metrics_ref.py::parent_fit (a
model compiled without metrics; captured and eager steps, with and without sample weights).  It was run on an MI355X
on the commit BEFORE compile(metrics=) existed (bbeea17, "Training: device-side learning rate, schedules, global clip,
decay"), so tests/test_gpu_metrics.py::test_fit_without_metrics_is_the_parent_run_bit_for_bit pins what a fit without
metrics computed there.  Every run is made three times and must repeat its own bits before it is written.

    python tests/golden/make_metrics_golden.py [OUT.npz]
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parent))
import metrics_ref as MR  # noqa: E402

out = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / MR.GOLDEN
rec = {"commit": np.array("bbeea17")}
for tag, graph, weighted in MR.PARENT_RUNS:
    loss, w = MR.parent_fit(graph, weighted)
    for _ in range(2):
        loss2, w2 = MR.parent_fit(graph, weighted)
        same = np.array_equal(loss, loss2) and all(np.array_equal(w[k], w2[k]) for k in w)
        print(f"{tag}: loss {[x.hex() for x in loss.tolist()]} repeats its bits: {same}", flush=True)
        assert same, f"{tag}: two runs of one build differ"
    rec[f"{tag}/loss"] = loss
    for k, v in w.items():
        rec[f"{tag}/w/{k}"] = np.asarray(v)
out.parent.mkdir(parents=True, exist_ok=True)
np.savez_compressed(out, **rec)
print(f"wrote {out} ({out.stat().st_size} bytes)")
