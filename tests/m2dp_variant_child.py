"""Child of tests/test_gpu_m2dp_match_edges.py::test_ab_switches_give_the_model_bits: the A/B switches of launch_m2dp_match_h (PR_M2_QTB,
PR_M2_WAVES) are function-static getenv()s, read at the first launch of a process, so each setting needs a process of its own.

    python m2dp_variant_child.py ARITH OUT.npz

runs the exact grid of m2dp_match_cases.py in the arithmetic ARITH at the shapes SHAPES through Matcher("m2dp") and writes both distance
matrices of every shape to OUT.npz (p_<m>_<n>, i_<m>_<n>).  The parent compares them with the model; nothing is judged here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

SHAPES = ((33, 65), (97, 1031), (9, 520))


def main(arith, out):
    import torch
    import m2dp_match_cases as M
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import Matcher
    q, db = M.cases(arith)
    mt = Matcher("m2dp", M.N_Q, M.N_DB, ctx=api.Context(0, sc_arith=arith))
    res = {}
    for m, n in SHAPES:
        mt.pack_database(torch.from_numpy(np.array(db[:4 * n])).cuda())
        mt.local_phase1(torch.from_numpy(np.array(q[:4 * m])).cuda())
        torch.cuda.synchronize()
        d_p, d_i = mt.distances()
        res[f"p_{m}_{n}"], res[f"i_{m}_{n}"] = d_p.cpu().numpy().copy(), d_i.cpu().numpy().copy()
    mt.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
