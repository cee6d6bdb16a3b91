"""A fresh process for the wide encoder's launch overrides (IMPNN_WIDE_NO_DIRECT, IMPNN_WIDE_TILE_ROWS,
IMPNN_WIDE_X3_BIG: the library reads each once per process, in choose_launch of csrc/encoder_wide.hip).
tests/test_gpu_wide_fuzz.py starts it with the overrides in its environment:

    python wide_child.py OUT.npz CASE:D [CASE:D ...]

It builds the cases of tests/wide_cases.py, runs both wide modes through encode_pooled(fused=True) - twice, the second
time on a workspace filled with 0xff bytes - and writes the pooled states to OUT.npz under "<case>/<D>/<mode>/cat|an"."""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
for p in (str(HERE), str(HERE.parent)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import wide_cases as WC  # noqa: E402
from ionic_mpnn_amd import model as MM  # noqa: E402
from ionic_mpnn_amd import ops  # noqa: E402


def run_case(case, mode, device):
    """(cat, an) pooled states of the whole case in `mode`, as float32 arrays."""
    m = MM.build_model(case.Va, case.Vb, atom_dim=case.D, bond_dim=case.K, num_steps=case.S, device=device)
    m.load_weights(case.weights)
    m.encoder_mode = mode
    assert m.resolve_encoder_mode(case.N, case.E) == mode
    d = {k: torch.from_numpy(np.array(v)).to(device) for k, v in case.inputs.items()}
    first = [t.cpu().numpy() for t in m.encode_pooled(d, fused=True)]
    # Once more with every byte of the encoder workspaces set to 0xff (NaN as a float, -1 as an index): a row of `agg`
    # that is read without having been written this call - a source that wide_place names and wide_reduce skips - would
    # otherwise read the zeros of fresh memory and pass.  The second run is the result; both must be the same bits.
    torch.cuda.synchronize()
    for ws in ops._workspaces.values():
        ws.fill_(0xFF)
    pc, pa = [t.cpu().numpy() for t in m.encode_pooled(d, fused=True)]
    for a, b, p in ((first[0], pc, "cat"), (first[1], pa, "an")):
        same = a.view(np.uint32) == b.view(np.uint32)
        assert same.all(), (f"{case.name} D={case.D} {mode} {p}: the result depends on what the workspace held before "
                            f"the call, in molecules {np.flatnonzero(~same.all(axis=1))[:12]}")
    return pc, pa


def main(argv):
    out, specs = argv[1], argv[2:]
    assert torch.cuda.is_available(), "wide_child.py needs a GPU"
    device = torch.device("cuda:0")
    res = {}
    for spec in specs:
        name, D = spec.split(":")
        case = WC.build(name, int(D))
        for mode in WC.MODES:
            res[f"{name}/{D}/{mode}/cat"], res[f"{name}/{D}/{mode}/an"] = run_case(case, mode, device)
    np.savez(out, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
