"""
montecarlo.enumerate_sharded for the two post-selected gadgets on the CPU: two torch.distributed (gloo) processes each enumerate
their shard of every weight's rank range with the host statement (local_fn) and all-reduce the counts; every rank must end with
the unsharded PostSelectedStrata.  tests/test_sharding_gloo.py's pattern: what is under test is the sharding arithmetic, the field
count taken from the part, and the collective, which are the same code on RCCL.
"""
import os
import socket
import sys

import numpy as np
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [0, 1, 2]


def _gadgets():
    from oracle import cpu_ref
    from quantum_css_codes_amd import ec_noise, ft_noise
    h = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
    code = cpu_ref.CSSCode(h, h)
    return ec_noise.ECCircuit(code, 2), ft_noise.FTProgram(code, "X")


def _host(gadget, weights, first_rank, count):
    return gadget.enumerate_strata(weights, first_rank=first_rank, count=count, host=True)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from quantum_css_codes_amd import montecarlo
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for name, gadget in zip(("ec", "ft"), _gadgets()):
        got = montecarlo.enumerate_sharded(gadget, WEIGHTS, local_fn=_host)
        assert isinstance(got, montecarlo.PostSelectedStrata) and got.nb == gadget.num_locations
        out[name + "_fields"] = np.array(got.fields)
        for w, counts in zip(got.weights, got.counts):
            out["%s_%d" % (name, w)] = counts
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def test_two_rank_enumeration_equals_the_unsharded_strata(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    from quantum_css_codes_amd import ec_noise, ft_noise
    for name, gadget, fields in zip(("ec", "ft"), _gadgets(), (ec_noise.EC_FIELDS, ft_noise.FT_FIELDS)):
        whole = gadget.enumerate_strata(WEIGHTS, host=True)
        for rank in (0, 1):                                   # every rank holds the whole strata
            got = np.load(tmp_path / ("rank%d.npz" % rank))
            assert tuple(got[name + "_fields"]) == fields
            for w, counts in zip(whole.weights, whole.counts):
                assert counts.shape == (w + 1, w + 1, len(fields)) and np.array_equal(got["%s_%d" % (name, w)], counts), (name, rank, w)
        assert int(whole.counts[2][:, :, 0].sum()) > 0
