"""Equity of states that already live in HBM as torch tensors -- no host round trip.

For pipelines that keep observations on the GPU (batched self-play, a policy network consuming the equity): the
queries are packed by torch ops on the current stream, evaluated by mcq_eval_batch_device on that same stream and
the result stays a device tensor, so nothing synchronises with the host.  torch is plumbing here (device memory,
streams); the evaluation is the library's HIP kernel.  Small batches (<= 1024 states) are cut into sub-tasks by
the prep kernel on the device.

    equity, tallies = get_equity_batch_torch(hole, board, n_players, runs, seed=1)

hole [B,2] uint8 card ids, board [B,5] uint8 (255 = empty slot, any position), n_players int or [B] uint8,
runs int or [B] int32 -- all on the same CUDA (HIP) device.  equity: float64 [B]; tallies: int64 [B,13] with
columns runs, passes, win, tie, by_type[9] (include/mcq.h mcq_result).  Query i runs under id first_query_id + i:
the numbers equal Engine.eval_batch / get_equity_batch on the same inputs, bit for bit.
ties="split": equity is hero's expected share of the pot (a tie among k hands counts 1/k), tallies int64 [B,22] with
nine more columns tie_ways[k - 2], k = 2..10 (mcq_result_ways) -- both computed on the device.
"""
import numpy as np
import torch

from . import _lib

_engines = {}


def _engine(index):
    if index not in _engines:
        _engines[index] = _lib.Engine(index)
    return _engines[index]


def pack_queries_torch(hole, board, n_players, runs):
    """mcq_query records ([B,16] uint8, on the inputs' device) from tensors; the table cards are left-packed."""
    dev = hole.device
    B = hole.shape[0]
    hole = hole.to(torch.uint8).reshape(B, 2)
    board = board.to(torch.uint8).reshape(B, 5)
    present = board != 255
    order = torch.argsort((~present).to(torch.uint8), dim=1, stable=True)
    packed = torch.gather(board, 1, order)
    nb = present.sum(1).to(torch.uint8)
    packed = torch.where(torch.arange(5, device=dev)[None, :] < nb[:, None], packed, torch.zeros_like(packed))
    q = torch.zeros((B, 16), dtype=torch.uint8, device=dev)
    q[:, 0:2] = hole
    q[:, 2:7] = packed
    q[:, 7] = nb
    q[:, 8] = torch.as_tensor(n_players, device=dev).to(torch.uint8).expand(B)
    r = torch.as_tensor(runs, device=dev).to(torch.int64).expand(B)
    for k in range(4):                                   # little-endian u32
        q[:, 12 + k] = ((r >> (8 * k)) & 255).to(torch.uint8)
    return q


def get_equity_batch_torch(hole, board, n_players, runs, seed=0, first_query_id=0, engine=None, ties="hero"):
    if ties not in ("hero", "split"):
        raise ValueError("ties must be 'hero' or 'split'")
    if not hole.is_cuda:
        raise ValueError("the tensors must live on the GPU (use get_equity_batch for host arrays)")
    eng = engine or _engine(hole.device.index if hole.device.index is not None else torch.cuda.current_device())
    q = pack_queries_torch(hole, board, n_players, runs)
    if ties == "split":
        out = torch.empty((q.shape[0], 22), dtype=torch.int64, device=q.device)
        eng.eval_batch_device_ways(q.data_ptr(), q.shape[0], seed, out.data_ptr(), first_query_id=first_query_id,
                                   stream=torch.cuda.current_stream(q.device).cuda_stream)
        q.record_stream(torch.cuda.current_stream(q.device))
        k = torch.arange(2, 11, dtype=torch.float64, device=q.device)
        share = out[:, 2].to(torch.float64) + (out[:, 13:22].to(torch.float64) / k).sum(1)
        return share / out[:, 0].clamp(min=1).to(torch.float64), out
    out = torch.empty((q.shape[0], 13), dtype=torch.int64, device=q.device)
    eng.eval_batch_device(q.data_ptr(), q.shape[0], seed, out.data_ptr(), first_query_id=first_query_id,
                          stream=torch.cuda.current_stream(q.device).cuda_stream)
    q.record_stream(torch.cuda.current_stream(q.device))
    equity = (out[:, 2] + out[:, 3]).to(torch.float64) / out[:, 0].clamp(min=1).to(torch.float64)
    return equity, out


def get_equity_matrix_torch(boards, dead=None, engine=None, want_tie=True):
    """The exact hand-against-hand matrices of a batch of boards as device tensors (mcq_exact_matrix_device; heads-up, the
    uniform law, 3 to 5 table cards per board).

    boards [n,5] uint8 card ids, 255 = empty slot (any position); dead (optional) [n] int64 masks, bit c = card id c is out
    of the deck.  The records are 16 bytes each and are validated on the host -- they are read back from the device if they
    live there --; the matrices never leave it: the kernels write them on the current stream of the boards' device (the
    current device for host tensors) and nothing waits for them.
    -> (win, tie, total): win, tie int16 [n,1326,1326] on the device, indexed by hand_index on both axes (tie None without
    want_tie), total int64 [n] on the host: win[i,h,g] + win[i,g,h] + tie[i,h,g] wherever h and g can both be dealt."""
    index = boards.device.index if boards.is_cuda and boards.device.index is not None else torch.cuda.current_device()
    device = torch.device("cuda", index)
    b = boards.detach().to("cpu", torch.uint8).reshape(-1, 5).numpy()
    n = b.shape[0]
    q = np.zeros(n, _lib.MATRIX_QUERY_DTYPE)
    for i in range(n):                                   # the table cards left-packed
        cards = b[i][b[i] != 255]
        q["board"][i, :len(cards)] = cards
        q["n_board"][i] = len(cards)
    if dead is not None:
        d = dead.detach().to("cpu", torch.int64).reshape(-1).numpy()
        if d.shape[0] != n:
            raise ValueError("one dead mask per board")
        q["dead"] = d.astype(np.uint64)
    eng = engine or _engine(index)
    win = torch.empty((n, _lib.HAND_ROWS, _lib.HAND_ROWS), dtype=torch.int16, device=device)
    tie = torch.empty_like(win) if want_tie else None
    total = eng.exact_matrix_device(q, win.data_ptr(), tie.data_ptr() if want_tie else 0,
                                    stream=torch.cuda.current_stream(device).cuda_stream)
    return win, tie, torch.from_numpy(total.astype(np.int64))
