"""Child of tests/test_gpu_snapshot.py::test_file_round_trip_across_processes: a process of its own that never saw the saved state.

    python snapshot_child.py SPEC.json FILE.snap

creates its own handles for the spec (snapshot_rig.Rig), loads FILE.snap into them and prints ONE JSON line: the load's info, the
sha256 of the live rows of every buffer and of every state, and the sha256 of the blob a device pack of the restored state gives.  The
parent compares them with its own; nothing is judged here."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import snapshot_np as sp          # noqa: E402
import snapshot_rig               # noqa: E402


def digests(state):
    """{part.array: sha256 of the live rows} and {part.state: ...} of a snapshot_np state"""
    out = {}
    for p, part in enumerate(state):
        n, pts = sp.counts(part)
        for name, bpr, which in part["sections"]:
            rows = pts if which == "pts" else (n + 1 if which == "n1" else n)
            out[f"{p}.{name}"] = hashlib.sha256(part["arrays"][name].reshape(-1).view("u1")[:rows * bpr].tobytes()).hexdigest()
        out[f"{p}.state"] = hashlib.sha256(part["state"].tobytes()).hexdigest()
    return out


def main():
    spec = json.load(open(sys.argv[1]))
    rig = snapshot_rig.Rig(spec)
    info = rig.snap.load(sys.argv[2])
    state = rig.download()
    raw, pinfo = rig.pack()
    rig.intact()
    rig.close()
    print(json.dumps(dict(info=info.tolist(), digests=digests(state), pack_info=pinfo.tolist(),
                          blob=hashlib.sha256(raw[:int(pinfo[0])].tobytes()).hexdigest())))


if __name__ == "__main__":
    main()
