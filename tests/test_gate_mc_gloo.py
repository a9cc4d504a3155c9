"""
montecarlo.gate_error_rates_sharded for the two post-selected gadgets on the CPU: four torch.distributed (gloo) processes each draw
their shard of the sample range with the host statement (local_fn) and all-reduce the F counts; every rank must end with the one-rank
counts.  tests/test_gate_strata_gloo.py's pattern: what is under test is the sharding arithmetic, the fields taken from the part, and
the collective, which are the same code on RCCL.
"""
import json
import os
import socket
import sys

import numpy as np
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 4
SAMPLES, FIRST = 4003, (1 << 40) + 10                         # no multiple of four: the first ranks take the extra samples
P1, P2 = 2e-3, 3e-3
SEED = 20261020


def _gadgets():
    from oracle import cpu_ref
    from quantum_css_codes_amd import ec_noise, ft_noise
    h = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
    code = cpu_ref.CSSCode(h, h)
    return ec_noise.ECCircuit(code, 2), ft_noise.FTProgram(code, "X")


def _host(gadget, num_samples, p1, p2, seed, first_sample):
    return gadget.gate_error_rates(num_samples, p1, p2, seed=seed, first_sample=first_sample, host=True)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from quantum_css_codes_amd import montecarlo
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for name, gadget in zip(("ec", "ft"), _gadgets()):
        out[name] = montecarlo.gate_error_rates_sharded(gadget, SAMPLES, P1, P2, SEED, FIRST, local_fn=_host)
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


def test_four_rank_gate_error_rates_equal_the_one_rank_counts(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(WORLD, port, str(tmp_path)), nprocs=WORLD, join=True)
    from quantum_css_codes_amd import ec_noise, ft_noise, montecarlo
    for name, gadget, fields in zip(("ec", "ft"), _gadgets(), (ec_noise.EC_FIELDS, ft_noise.FT_FIELDS)):
        whole = _host(gadget, SAMPLES, P1, P2, SEED, FIRST)
        assert montecarlo.gate_error_rates_sharded(gadget, SAMPLES, P1, P2, SEED, FIRST, local_fn=_host) == whole   # no process group
        for rank in range(WORLD):                             # every rank holds the whole counts
            with open(tmp_path / ("rank%d.json" % rank)) as f:
                got = json.load(f)[name]
            assert list(got) == list(fields) + ['samples'] and got == whole, (name, rank)
        assert whole['samples'] == SAMPLES and 0 < whole['accepted'] < SAMPLES
