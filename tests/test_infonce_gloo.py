"""CPU, world size 2 over gloo: the multi-rank path of models/infoNCE.py.  Gather / shuffle / un-shuffle hands every rank its own
rows back, the permutation is rank 0's, and the enqueue writes both ranks' keys (and labels) in rank order."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
    try:
        import test_infonce_cpu as tc
        from video_similarity_search_amd.models.infoNCE import concat_all_gather
        B = tc.B
        m = tc.make("UberNCE", seed=4).train()                       # the same weights on both ranks
        # gather: rank order
        mine = torch.full((2, 3), float(rank))
        assert torch.equal(concat_all_gather(mine), torch.cat([torch.zeros(2, 3), torch.ones(2, 3)]))
        # shuffle: every rank gets its slice of rank 0's permutation; un-shuffle returns its own rows
        x = (torch.arange(B * 3, dtype=torch.float64).view(B, 3) + 100 * rank)
        torch.manual_seed(10 + rank)                                 # different generators: the broadcast decides
        xs, perm = m._batch_shuffle_ddp(x)
        both = torch.cat([torch.arange(B * 3, dtype=torch.float64).view(B, 3) + 100 * r for r in range(world)])
        assert sorted(perm.tolist()) == list(range(world * B)) and torch.equal(xs, both[perm.view(world, -1)[rank]])
        perms = concat_all_gather(perm.view(1, -1))
        assert torch.equal(perms[0], perms[1])
        assert torch.equal(m._batch_unshuffle_ddp(xs, perm), x)
        # a training step: both ranks' keys and labels enter the queue in rank order (the trunk has no BatchNorm: a key does not
        # depend on which rank encoded it)
        blocks = [tc.blocks(1, seed=30 + r)[0] for r in range(world)]
        labels = [torch.tensor([r, r + 1, r + 2, r + 3]) for r in range(world)]
        with torch.no_grad():
            keys = [m._encode(m.encoder_k, b[:, 1].contiguous()) for b in blocks]     # before the step: the EMA moves nothing (k == q)
        logits, mask = m(blocks[rank], labels[rank])
        assert tuple(logits.shape) == (B, tc.K + 1) and int(m.queue_ptr) == world * B
        got = m.queue.t()[:world * B]
        assert (got - torch.cat(keys)).abs().max().item() < 1e-12
        assert torch.equal(m.queue_label[:world * B], torch.cat(labels)) and (m.queue_label[world * B:] == -1).all()
        logits.sum().backward()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), queue=m.queue.numpy(), perm=perm.numpy())
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(tmp_path / f"r{r}.npz") for r in range(2))
    assert np.array_equal(r0["queue"], r1["queue"]) and np.array_equal(r0["perm"], r1["perm"])


def _ddp_worker(rank, world, port, out_dir):
    import contextlib
    import io
    import sys
    import types
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
    try:
        import test_infonce_cpu as tc
        from torch.nn.parallel import DistributedDataParallel
        from video_similarity_search_amd.misc.distributed_helper import data_parallel
        from video_similarity_search_amd.models.infoNCE import concat_all_gather
        from video_similarity_search_amd.online_train import UberNCE_train_epoch
        blk = tc.blocks(1, seed=40 + rank)[0]                            # every rank its own clips and labels
        six = blk.transpose(1, 2).reshape(tc.B, 6, *tc.CLIP[1:])
        item = ([six[:, :3].numpy(), six[:, 3:].numpy()], [torch.tensor([rank, 1, 2, rank])] * 2, torch.arange(tc.B))

        def epoch_step(wrap, arch, cls):
            m = tc.make(cls, seed=4)                                       # the same weights on both ranks
            model = wrap(m) if wrap is not None else m
            opt = torch.optim.SGD(m.encoder_q.parameters(), lr=0.1)
            cfg = tc.epoch_cfg(arch, None)
            cfg.NUM_GPUS = world if wrap is not None else 1
            with contextlib.redirect_stdout(io.StringIO()):
                UberNCE_train_epoch(tc.Loader([item], world * tc.B), model, None, opt, 0, cfg, False, "cpu", rank == 0, fused=True)
            return (torch.cat([p.grad.reshape(-1) for p in m.encoder_q.parameters()]),
                    torch.cat([p.detach().reshape(-1) for p in m.encoder_q.parameters()]))

        for arch, cls in (("uber_nce", "UberNCE"), ("info_nce", "InfoNCE")):
            g_local, w_local = epoch_step(None, arch, cls)                 # no wrapper: each rank's own gradient
            for wrap in (lambda m: DistributedDataParallel(m), lambda m: data_parallel(m)):
                g, w = epoch_step(wrap, arch, cls)
                both_g, both_w = concat_all_gather(g.view(1, -1)), concat_all_gather(w.view(1, -1))
                assert torch.equal(both_g[0], both_g[1]) and torch.equal(both_w[0], both_w[1])     # the fused step went through the wrapper
                assert not torch.equal(g, g_local) and not torch.equal(w, w_local)
                mean_local = concat_all_gather(g_local.view(1, -1)).mean(0)
                assert (g - mean_local).abs().max().item() <= 1e-12 * max(1.0, mean_local.abs().max().item())
        open(os.path.join(out_dir, f"ok{rank}"), "w").close()
    finally:
        torch.distributed.destroy_process_group()


def test_wrapped_fused_epoch_step_synchronises_gradients(tmp_path):
    """UberNCE_train_epoch(fused=True) on a DistributedDataParallel model (torch's wrapper and data_parallel): both ranks end the
    step with bit-equal query-encoder gradients and weights, the mean of the two ranks' own gradients, not their own"""
    mp.spawn(_ddp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "ok0") and os.path.exists(tmp_path / "ok1")
