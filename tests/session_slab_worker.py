"""One rank of a row-slab job that loads a whole-grid handle's state twice, side by side: once from the plain snapshot, once from the session file saved at the same
moment (euler_load_state takes the core of a version-4 file and ignores its chunks, docs/session.md).  Every own row, marker, key and counter must be the same, at once and
a frame later.  Rank 0 prints one JSON line.

  session_slab_worker.py X Y SNAPSHOT SESSION"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.distributed as dist

from slab_observers_worker import make_slab, state_of


def main():
    X, Y, snap, session = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, world = dist.get_rank(), dist.get_world_size()
    a, ca = make_slab(X, Y, rank, world, False, False, 0)
    b, cb = make_slab(X, Y, rank, world, False, False, 0)
    a.load_state(snap); b.load_state(session)

    def differ():
        sa, sb = state_of(a, False), state_of(b, False)
        every = [None] * world
        dist.all_gather_object(every, sorted(k for k in sa if sa[k] != sb[k]))
        return sorted({k for e in every for k in e})

    out = {"world": world, "differ": differ(), "markers": int(a.stats().n_markers), "time": [a.time, b.time]}
    a.step(); b.step()
    out["differ_after_a_frame"] = differ()
    for c in (ca, cb):
        if c.error:
            raise RuntimeError(c.error)
    if rank == 0:
        print(json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
