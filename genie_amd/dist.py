"""Source-node sharding of the product graph across the GPUs of one node.

One process per GPU (`torch.distributed`, backend "nccl" = RCCL over xGMI on ROCm). Product nodes are `(g, s)`; rank r
OWNS a contiguous block of a space-filling-curve order of the source nodes and therefore the rows `[g*S, (g+1)*S)` of
every `[P, .]` tensor. Station-neighbour gathers and the Bipartite station sum are local. Source-neighbour gathers need
rows of neighbour source nodes owned elsewhere (the HALO):

* layer 1 recomputes every neighbour's hidden state from its raw 8 input floats, so the halo of layer 1 is just the
  halo nodes' `Slice/Mask` rows, which every rank loads/embeds itself (input distribution, no collective);
* layer 2 gathers the projected operand `wv` (15 channels, 64-B rows): ONE all-to-all of halo rows per window, issued on a
  communication stream as soon as stage 1 has produced the rows other ranks need, and overlapped with the rest of stage 1 and
  with stage 2 of the source nodes that have no halo neighbour;
* the `[G, 15]` Bipartite output is all-gathered (one `all_gather_into_tensor` + one index op) and the G-sized
  SpatialAggregation / read-out kernels run replicated, on a tail stream under the next window's P-sized kernels.

How the overlap is arranged: a rank's owned source nodes fall into the classes SEND (some other rank lists them as a
neighbour) and NEED (they have a neighbour owned elsewhere). The local processing order is
`[SEND only | SEND and NEED | NEED only | interior]`, each class in space-filling-curve order, so that
  stage 1 = range [0, n_send) -> all-to-all starts -> range [n_send, n_own)
  stage 2 = the two ranges without NEED nodes -> wait for the halo rows -> the NEED range
are contiguous sub-ranges of that order (`genie_da_stage1_range`, `genie_da_stage2_partials_range`).

The reference has no multi-GPU code at all (`process_config.yaml:66 parallel_processing: False`); the layout
sharded here is its product-node numbering `p = g * n_sta + s` (`process_utils.py:720-722`).
"""
import numpy as np
import torch

from . import engine


class ShardRows(object):
    """Rows of a per-product-node tensor in a rank's LOCAL order: the S-row blocks of its owned source nodes (space-filling-curve
    order), then of its halo nodes (`ShardPlan.ext_global`), or of the owned nodes only (`own_only`). What the sharded drop-in model
    produces (`embed_window`, `node_rows`) and accepts in place of the reference's full `[P, C]` tensors -- a full tensor and a
    local one can have the same shape (world size 1), so the local form is a type of its own, never guessed from a shape."""
    __slots__ = ("t", "own_only")

    def __init__(self, t, own_only=False):
        self.t, self.own_only = t, bool(own_only)

    @property
    def shape(self):
        return self.t.shape


def resolve_shard(process_group=None, shard=None):
    """(rank, world, group) of a sharded model, or None for an unsharded one. `process_group`: a `torch.distributed` group, or True
    for the default group; `shard` = (rank, world) overrides what the group reports (and is all there is without a group: a virtual
    rank, whose collectives the caller replaces -- `bench.py --emulate-world`)."""
    if process_group is None and shard is None:
        return None
    import torch.distributed as dist
    group = None
    if process_group is not None and process_group is not True:
        group = process_group
    if shard is not None:
        rank, world = int(shard[0]), int(shard[1])
    else:
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("process_group given but torch.distributed is not initialised (init_process_group first)")
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    if not 0 <= rank < world:
        raise ValueError("shard = (rank, world) needs 0 <= rank < world")
    return rank, world, group


class ShardPlan(object):
    """Static plan for one rank (pure numpy, deterministic and identical logic on every rank).

    A_src_src: int [2, E] global source graph (row 0 = neighbour j, row 1 = centre i, in-edges grouped by centre).
    order:     permutation of the G source nodes (space-filling-curve order); rank r owns order[lo_r:hi_r].
    Local numbering on a rank: owned nodes 0..n_own-1 (in `order` order), then halo nodes grouped by owner rank.
    """

    def __init__(self, A_src_src, n_grid, world, rank, order=None):
        A = np.asarray(A_src_src)
        G, W = int(n_grid), int(world)
        order = np.arange(G) if order is None else np.asarray(order, dtype=np.int64)
        assert order.shape == (G,) and np.array_equal(np.sort(order), np.arange(G)), "order must be a permutation of the source nodes"
        self.n_grid, self.world, self.rank = G, W, int(rank)
        bounds = [(G * r) // W for r in range(W + 1)]
        self.bounds = bounds
        owner = np.empty(G, dtype=np.int64)
        for r in range(W):
            owner[order[bounds[r]:bounds[r + 1]]] = r
        self.owner = owner
        self.owned = [order[bounds[r]:bounds[r + 1]].copy() for r in range(W)]          # global ids per rank
        j, i = A[0].astype(np.int64), A[1].astype(np.int64)
        # need[r][q] = sorted global ids owned by q that appear as neighbours of nodes owned by r
        cross = owner[i] != owner[j]
        ci, cj = owner[i[cross]], j[cross]
        self.need = [[np.zeros(0, dtype=np.int64)] * W for _ in range(W)]
        for r in range(W):
            nb = np.unique(cj[ci == r])
            onb = owner[nb]
            self.need[r] = [nb[onb == q] if q != r else np.zeros(0, dtype=np.int64) for q in range(W)]
        me = self.rank
        self.own_global = self.owned[me]
        self.n_own = int(self.own_global.size)
        self.halo_global = np.concatenate([self.need[me][q] for q in range(W)]) if W > 1 else np.zeros(0, dtype=np.int64)
        self.n_halo = int(self.halo_global.size)
        self.n_ext = self.n_own + self.n_halo
        self.ext_global = np.concatenate([self.own_global, self.halo_global])
        g2l = -np.ones(G, dtype=np.int64)
        g2l[self.ext_global] = np.arange(self.n_ext)
        self.global_to_local = g2l
        # local CSR of the owned nodes (in-edges in the original edge order), columns in local numbering
        order_e = np.argsort(i, kind="stable")
        js, is_ = j[order_e], i[order_e]
        start = np.searchsorted(is_, self.own_global, side="left")
        stop = np.searchsorted(is_, self.own_global, side="right")
        deg = stop - start
        rowptr = np.zeros(self.n_own + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum(deg)
        take = np.repeat(start - rowptr[:-1], deg) + np.arange(int(rowptr[-1]))        # edge positions, row by row
        col = g2l[js[take]] if take.size else np.zeros(0, dtype=np.int64)
        assert (col >= 0).all(), "halo is incomplete"
        self.src_rowptr = rowptr.astype(np.int32)
        self.src_col = col.astype(np.int32)
        # what this rank sends to q = the rows q needs from it, as LOCAL owned indices, in q's halo order
        self.send_local = [g2l[self.need[q][me]] if q != me else np.zeros(0, dtype=np.int64) for q in range(W)]
        self.send_counts = [int(x.size) for x in self.send_local]
        self.recv_counts = [int(self.need[me][q].size) for q in range(W)]
        # classes of owned nodes and the local processing order [SEND only | SEND and NEED | NEED only | interior]
        send = np.zeros(self.n_own, dtype=bool)
        if W > 1:
            send[np.concatenate(self.send_local).astype(np.int64)] = True
        need = np.zeros(self.n_own, dtype=bool)
        if col.size:
            row_of = np.repeat(np.arange(self.n_own), deg)
            need[row_of[col >= self.n_own]] = True
        loc = np.arange(self.n_own)
        parts = [loc[send & ~need], loc[send & need], loc[~send & need], loc[~send & ~need]]
        self.proc_order = np.concatenate(parts).astype(np.int32)
        c = np.cumsum([0] + [p.size for p in parts])
        self.r_send = (int(c[0]), int(c[2]))          # positions of the SEND nodes in proc_order
        self.r_need = (int(c[1]), int(c[3]))          # positions of the NEED nodes
        self.n_send_nodes, self.n_need_nodes = int(send.sum()), int(need.sum())

    def halo_fraction(self):
        return self.n_halo / max(1, self.n_own)


class SubgraphShardPlan(object):
    """Static plan for one rank of an IRREGULAR product graph (`use_subgraph`) sharded over source nodes (pure numpy, the same logic on
    every rank). The product nodes are rows grouped by source node (`seg_rowptr` [G + 1]); `src_csr` / `sta_csr` = (rowptr [n_prod + 1],
    col) are the product-level CSRs (in-edges per row, in the edge order the unsharded context takes them in).

    Ownership is by source node, in `order`, as in `ShardPlan`: rank r owns order[lo_r:hi_r] and with them their rows. The halo is
    RAGGED: exactly the rows of source nodes owned elsewhere that appear as a neighbour in the source CSR of an owned row, grouped by
    owner, in the owner's local row order. Local row numbering: the owned rows, source node after source node in the processing order
    `[SEND only | SEND and NEED | NEED only | interior]` (a node is SEND when one of its rows is in another rank's halo, NEED when one of
    its rows has a neighbour owned elsewhere), then the halo rows. A range of processing positions is therefore a range of rows.
    Counts (`send_counts`, `recv_counts`) are in rows.

    own_global  [n_own]   owned source nodes in `order` order (what `gather_index` places; `proc_order` indexes it)
    own_proc    [n_own]   owned source nodes in processing order = the local node numbering of the rank's HIP context
    seg_rowptr  [n_own+1] local row range of every local node
    own_rows / halo_rows / ext_rows: global row ids of the local rows
    sta_rowptr, sta_col, src_rowptr, src_col: local product-level CSRs of the owned rows, columns = local row ids
    send_rows[q]: local owned rows this rank sends to q, in q's halo order."""

    def __init__(self, seg_rowptr, src_csr, sta_csr, n_grid, world, rank, order=None):
        seg = np.asarray(seg_rowptr, dtype=np.int64)
        G, W, me = int(n_grid), int(world), int(rank)
        n_prod = int(seg[-1])
        assert seg.shape == (G + 1,) and seg[0] == 0 and (np.diff(seg) >= 0).all(), "seg_rowptr: row ranges of the G source nodes"
        order = np.arange(G) if order is None else np.asarray(order, dtype=np.int64)
        assert order.shape == (G,) and np.array_equal(np.sort(order), np.arange(G)), "order must be a permutation of the source nodes"
        self.n_grid, self.world, self.rank, self.n_prod = G, W, me, n_prod
        bounds = [(G * r) // W for r in range(W + 1)]
        self.bounds = bounds
        owner = np.empty(G, dtype=np.int64)
        for r in range(W):
            owner[order[bounds[r]:bounds[r + 1]]] = r
        self.owner = owner
        self.owned = [order[bounds[r]:bounds[r + 1]].copy() for r in range(W)]
        n_rows = np.diff(seg)
        src_of = np.repeat(np.arange(G, dtype=np.int64), n_rows)
        row_owner = owner[src_of]
        rp, col = np.asarray(src_csr[0], dtype=np.int64), np.asarray(src_csr[1], dtype=np.int64)
        srp, scol = np.asarray(sta_csr[0], dtype=np.int64), np.asarray(sta_csr[1], dtype=np.int64)
        assert rp.shape == (n_prod + 1,) and srp.shape == (n_prod + 1,), "product-level CSRs over the n_prod rows"
        assert col.size == 0 or (col.min() >= 0 and col.max() < n_prod), "source CSR column outside the product nodes"
        assert scol.size == 0 or (src_of[scol] == np.repeat(src_of, np.diff(srp))).all(), "a station neighbour is a row of the same source node"
        centre = np.repeat(np.arange(n_prod, dtype=np.int64), np.diff(rp))
        cross = row_owner[centre] != row_owner[col]
        ci, cj = centre[cross], col[cross]
        # classes of every source node (of every rank: the owners' row orders are needed for the halo order)
        send_row = np.zeros(n_prod, dtype=bool)
        send_row[cj] = True
        need_row = np.zeros(n_prod, dtype=bool)
        need_row[ci] = True
        send_node = np.bincount(src_of, weights=send_row, minlength=G) > 0
        need_node = np.bincount(src_of, weights=need_row, minlength=G) > 0
        row_local = np.empty(n_prod, dtype=np.int64)         # position of a row in its OWNER's local list
        procs, rows_of = [], []
        for r in range(W):
            nodes = self.owned[r]
            s, n = send_node[nodes], need_node[nodes]
            loc = np.arange(nodes.size)
            parts = [loc[s & ~n], loc[s & n], loc[~s & n], loc[~s & ~n]]
            po = np.concatenate(parts).astype(np.int64)
            procs.append((po, np.cumsum([0] + [p.size for p in parts])))
            gp = nodes[po]
            cnt = n_rows[gp]
            off = np.concatenate(([0], np.cumsum(cnt)))
            rows = np.repeat(seg[gp] - off[:-1], cnt) + np.arange(int(off[-1]))
            row_local[rows] = np.arange(rows.size)
            rows_of.append(rows)
        # need[r][q]: global rows owned by q that rows of r list as neighbours, in q's local row order
        self.need = []
        cr = row_owner[ci]
        for r in range(W):
            nb = np.unique(cj[cr == r])
            nb = nb[np.argsort(row_local[nb], kind="stable")]
            onb = row_owner[nb]
            self.need.append([nb[onb == q] for q in range(W)])
        po, c = procs[me]
        self.own_global = self.owned[me]
        self.n_own = int(self.own_global.size)
        self.proc_order = po.astype(np.int32)
        self.own_proc = self.own_global[po]
        self.r_send, self.r_need = (int(c[0]), int(c[2])), (int(c[1]), int(c[3]))
        self.n_send_nodes, self.n_need_nodes = int(c[2] - c[0]), int(c[3] - c[1])
        self.own_rows = rows_of[me]
        self.halo_rows = np.concatenate(self.need[me]) if W > 1 else np.zeros(0, dtype=np.int64)
        self.ext_rows = np.concatenate([self.own_rows, self.halo_rows])
        self.n_rows_own, self.n_rows_halo = int(self.own_rows.size), int(self.halo_rows.size)
        self.n_rows_ext = self.n_rows_own + self.n_rows_halo
        self.seg_rowptr = np.concatenate(([0], np.cumsum(n_rows[self.own_proc]))).astype(np.int32)
        g2l = -np.ones(n_prod, dtype=np.int64)
        g2l[self.ext_rows] = np.arange(self.n_rows_ext)
        self.row_to_local = g2l

        def local_csr(rowptr, cols):
            deg = (rowptr[1:] - rowptr[:-1])[self.own_rows]
            lrp = np.concatenate(([0], np.cumsum(deg)))
            take = np.repeat(rowptr[:-1][self.own_rows] - lrp[:-1], deg) + np.arange(int(lrp[-1]))
            lc = g2l[cols[take]] if take.size else np.zeros(0, dtype=np.int64)
            assert (lc >= 0).all(), "halo is incomplete"
            return lrp.astype(np.int32), lc.astype(np.int32)
        self.src_rowptr, self.src_col = local_csr(rp, col)
        self.sta_rowptr, self.sta_col = local_csr(srp, scol)
        assert (self.sta_col < self.n_rows_own).all()
        self.send_rows = [g2l[self.need[q][me]] if q != me else np.zeros(0, dtype=np.int64) for q in range(W)]
        self.send_counts = [int(x.size) for x in self.send_rows]
        self.recv_counts = [int(x.size) for x in self.need[me]]

    def halo_fraction(self):
        return self.n_rows_halo / max(1, self.n_rows_own)


class Transport(object):
    """The two collectives of the sharded path. RCCL ("nccl") takes device buffers directly on the current stream; a process
    group without device collectives (gloo: the CPU tests and the several-processes-on-one-GPU test) is served by staging
    through host memory, which synchronises the calling stream -- test plumbing, not a data path."""

    def __init__(self, group=None, world=None, emulate=False):
        """`world`: the rank count of the plan the collectives serve. A process group of another size cannot carry them: a one-rank
        plan inside an N-rank job (a single-GPU leg of a multi-rank run) then runs without collectives -- pass an explicit one-rank
        `group` to exercise the RCCL path there --, any other mismatch is an error.
        `emulate`: ONE virtual rank of a `world`-rank plan alone on its GPU (`bench.py --emulate-world`): no peer exists, every
        collective is replaced by a device-to-device copy of the same number of bytes (this rank's own rows stand in for the peers'), so
        the kernels, sub-range launches, stream dependencies and buffer sizes are those of rank r at N = world and the RESULTS ARE NOT
        the model's output. For timing only."""
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.emulate = bool(emulate)
        self.world = int(world or 1)
        if self.emulate:
            self.on, self.device_collectives = False, False
            return
        self.on = dist.is_available() and dist.is_initialized()
        if self.on and world is not None and dist.get_world_size(group) != int(world):
            if int(world) != 1:
                raise ValueError("process group of %d ranks cannot serve a %d-rank shard plan" % (dist.get_world_size(group), int(world)))
            self.on = False
        self.device_collectives = self.on and dist.get_backend(group) == "nccl"

    def _no_group(self):
        """A collective of a plan of several ranks without a process group: the result would silently miss the peers' rows."""
        if self.world > 1:
            raise RuntimeError("a %d-rank shard plan needs an initialised torch.distributed process group for its collectives (or "
                               "emulate=True: one virtual rank timed alone, results meaningless)" % self.world)

    def all_to_all_rows(self, recv, send, recv_counts, send_counts):
        """recv [sum(recv_counts), C] <- send [sum(send_counts), C], row blocks grouped by peer."""
        if self.emulate:
            if recv.shape[0] and send.shape[0]:
                torch.index_select(send, 0, torch.arange(recv.shape[0], device=send.device) % send.shape[0], out=recv)
            return
        if not self.on:
            return self._no_group()
        if self.device_collectives or not send.is_cuda:
            self.dist.all_to_all_single(recv, send, output_split_sizes=recv_counts, input_split_sizes=send_counts, group=self.group)
            return
        r = torch.empty(tuple(recv.shape), dtype=recv.dtype)
        self.dist.all_to_all_single(r, send.cpu(), output_split_sizes=recv_counts, input_split_sizes=send_counts, group=self.group)
        recv.copy_(r)

    def halo_p2p_rows(self, recv, send, recv_counts, send_counts, rank, pack=None):
        """The halo exchange bucketed by destination: one (send, receive) pair per peer this rank really exchanges rows with, the
        largest transfer first, each pair its own group (`batch_isend_irecv`: on RCCL one fused send / receive per peer = per
        xGMI link, the pairs independent of each other). `pack(q, view)` fills the send rows of peer q right before that peer's
        transfer is posted, so the packing of peer q + 1 runs under the transfer of peer q. Same rows in the same places as
        `all_to_all_rows` (tests/test_dist_cpu.py: both forms over gloo)."""
        if self.emulate:
            so = np.concatenate(([0], np.cumsum(send_counts))).astype(np.int64)
            for q in range(len(send_counts)):
                if pack is not None and q != rank and send_counts[q]:
                    pack(q, send[so[q]:so[q + 1]])
            return self.all_to_all_rows(recv, send, recv_counts, send_counts)
        if not self.on:
            return self._no_group()
        dist = self.dist
        so = np.concatenate(([0], np.cumsum(send_counts))).astype(np.int64)
        ro = np.concatenate(([0], np.cumsum(recv_counts))).astype(np.int64)
        peers = [q for q in range(len(send_counts)) if q != rank and (send_counts[q] or recv_counts[q])]
        peers.sort(key=lambda q: -(send_counts[q] + recv_counts[q]))
        device = self.device_collectives or not send.is_cuda
        works, staged = [], []
        for q in peers:
            sv, rv = send[so[q]:so[q + 1]], recv[ro[q]:ro[q + 1]]
            if pack is not None and send_counts[q]:
                pack(q, sv)
            ops = []
            if not device:               # process group without device collectives: staged through host memory (test plumbing)
                sv, rh = sv.cpu(), torch.empty(tuple(rv.shape), dtype=rv.dtype)
                staged.append((rv, rh))
                rv = rh
            if send_counts[q]:
                ops.append(dist.P2POp(dist.isend, sv, q if self.group is None else dist.get_global_rank(self.group, q), self.group))
            if recv_counts[q]:
                ops.append(dist.P2POp(dist.irecv, rv, q if self.group is None else dist.get_global_rank(self.group, q), self.group))
            works += dist.batch_isend_irecv(ops)
        for w in works:
            w.wait()
        for rv, rh in staged:
            rv.copy_(rh)

    def all_gather_rows(self, out, x):
        """out [world, n, C] <- x [n, C] of every rank."""
        if self.emulate:
            out.copy_(x.unsqueeze(0).expand_as(out))
            return
        if not self.on:
            self._no_group()
            out[0].copy_(x)
            return
        if self.device_collectives:
            self.dist.all_gather_into_tensor(out.view(-1, x.shape[1]), x, group=self.group)
            return
        parts = [torch.empty(tuple(x.shape), dtype=x.dtype) for _ in range(out.shape[0])]
        self.dist.all_gather(parts, x.cpu(), group=self.group)
        out.copy_(torch.stack(parts))


    def all_gather_ragged(self, rows, count, timeout=60.0):
        """Every rank's first `count` (device int32 [1]) rows of `rows` [cap, C], rank after rank: [sum of counts, C]. Counts first (one
        read-back on every rank), then the rows padded to the longest count; a rank with no row joins both collectives. On the device
        over RCCL; staged through the host over gloo, where each wait ends after `timeout` seconds."""
        if self.emulate or not self.on:
            if not self.emulate:
                self._no_group()
            return rows[: int(count.item())]
        import datetime
        dist, W, C = self.dist, self.world, rows.shape[1]
        if self.device_collectives:
            counts = torch.empty(W, dtype=count.dtype, device=count.device)
            dist.all_gather_into_tensor(counts, count, group=self.group)
            counts = counts.tolist()
            n_max = max(counts)
            if n_max == 0:
                return rows[:0]
            buf = rows.new_empty((W, n_max, C))
            dist.all_gather_into_tensor(buf.view(-1, C), rows[:n_max], group=self.group)
        else:
            wait = datetime.timedelta(seconds=float(timeout))
            parts = [torch.empty(1, dtype=count.dtype) for _ in range(W)]
            dist.all_gather(parts, count.cpu(), group=self.group, async_op=True).wait(wait)
            counts = [int(c) for c in parts]
            n_max = max(counts)
            if n_max == 0:
                return rows[:0]
            parts = [torch.empty((n_max, C), dtype=rows.dtype) for _ in range(W)]
            dist.all_gather(parts, rows[:n_max].cpu(), group=self.group, async_op=True).wait(wait)
            buf = torch.stack(parts).to(rows.device)
        return torch.cat([buf[r, : counts[r]] for r in range(W)])


def pointer_row_owners(a_edges, base, plan, n_sta, k=10):
    """Which rank owns each of the `k` product nodes a pick's time-pointer entry lists: `a_edges` flat table of global product-node ids
    (p = g * n_sta + s), `base` [n] the picks' entry numbers `ipick * l_dt + time bin` -> int64 [n, k] ranks. Pure numpy (the split the
    ranks' `genie_lslc_rows` calls make between them)."""
    e = np.asarray(a_edges).reshape(-1)[(np.asarray(base, dtype=np.int64).reshape(-1, 1) * k + np.arange(k)).reshape(-1)]
    return plan.owner[e.astype(np.int64) // int(n_sta)].reshape(-1, k)


def place_pick_rows(gathered, n_entries):
    """The all-gathered compact lists of `genie_lslc_rows` ([m, 32]: row, arrival, bits of the entry number) PLACED at their entry
    numbers in a zero table [n_entries, 32]. Every entry has one owner; adding instead would turn a -0.0 into +0.0."""
    table = gathered.new_zeros((int(n_entries), gathered.shape[1]))
    if gathered.shape[0]:
        keys = gathered[:, 31].contiguous().view(torch.int32).long()
        table.index_copy_(0, keys, gathered)
    return table


def shard_time_pointers(tl_own, own_global, n_sta, n_grid, transport, max_t=None, dt=1.0, k=10, win=10.0, candidates=None, merge=None):
    """The association heads' time-pointer tables of a source-node-sharded model from each rank's OWN travel-time rows: the tables of
    `engine.time_pointers_device` / `graph.time_pointers` over the whole product graph, bit for bit, the same on every rank.

    tl_own fp32 [n_own * n_sta, 2]: the rows of this rank's owned source nodes `own_global` in local node order. Every rank calls with the
    same n_sta, n_grid, max_t, dt, k, win. Two collectives over `transport`, joined by every rank whatever it owns:
      1. one [1, 2] float64 row per rank -- its largest travel time and whether it holds an inf / NaN -- so that `max_t=None` (the largest
         travel time of the WHOLE graph) and the verdict agree: a bad travel time on one rank raises ValueError on all of them, here,
         after the collective, and no rank waits for another in the next one;
      2. the ranks' candidate blocks: per (phase, station, time step) a rank's min(k, n_own) smallest keys (float64 distance, global
         product-node id), padded with a key that sorts last (`candidates`, default `engine.time_pointers_candidates`). A key among the
         k smallest of the station is among the k smallest of its owner, so the k smallest of the gathered world x k keys (`merge`,
         default `engine.time_pointers_merge`) are the station's.
    dt_partition is computed on the host as `time_pointers_device` computes it. `candidates` / `merge`: the two kernels' stand-ins with
    their signatures, for tensors that do not live on a GPU (tests/test_shard_time_pointers_cpu.py).
    Returns (A_edges_p, A_edges_s, dt_partition): int32 [n_sta * len(dt_partition) * min(k, n_grid)] each, and the float64 numpy steps."""
    k, n_sta, n_grid = int(k), int(n_sta), int(n_grid)
    if not 1 <= k <= engine.TIME_POINTERS_MAX_K:
        raise ValueError("time_pointers on a shard: 1 <= k <= %d required, got %d" % (engine.TIME_POINTERS_MAX_K, k))
    if n_sta < 1 or n_grid < 1 or n_sta * n_grid >= 2 ** 31:
        raise ValueError("time_pointers on a shard: 1 <= n_sta * n_grid < 2^31 required")
    if not float(dt) > 0.0:
        raise ValueError("time_pointers on a shard: dt > 0 required")
    own_global = np.asarray(own_global, dtype=np.int64)
    n_own = int(own_global.size)
    if tuple(tl_own.shape) != (n_own * n_sta, 2) or tl_own.dtype != torch.float32:
        raise ValueError("time_pointers on a shard: expected fp32 travel times [%d, 2] (owned rows), got %s" % (n_own * n_sta, tuple(tl_own.shape)))
    dev = tl_own.device
    mine = torch.tensor([[-np.inf, 0.0]], dtype=torch.float64, device=dev)
    if n_own:
        finite = torch.isfinite(tl_own)
        mine[0, 0] = torch.where(finite, tl_own, tl_own.new_full((), -np.inf)).max().double()      # (fp32 -> fp64: exact)
        mine[0, 1] = (~finite).any().double()
    every = mine.new_empty((transport.world, 1, 2))
    transport.all_gather_rows(every, mine)
    every = every.view(-1, 2).cpu().numpy()                  # the one read-back of the agreed constants
    if every[:, 1].any():
        raise ValueError("time_pointers on a shard: travel times must be finite (inf / NaN in the rows of rank(s) %s)"
                         % ", ".join(str(r) for r in np.nonzero(every[:, 1])[0]))
    if max_t is None:
        max_t = np.float32(every[:, 0].max())                # (the host function's `trv.max()`: an fp32 scalar)
    dt_partition = np.arange(-win, win + max_t + dt, dt)
    n_t = int(dt_partition.size)
    if n_t < 2:
        raise ValueError("time_pointers on a shard: dt_partition needs at least two time steps")
    k_tab = min(k, n_grid)
    dtp = torch.from_numpy(dt_partition).to(dev)
    node_global = torch.from_numpy(own_global.astype(np.int32)).to(dev)
    cand = (candidates or engine.time_pointers_candidates)(tl_own, n_sta, node_global, dtp, k_tab)
    cand_all = cand.new_empty((transport.world,) + tuple(cand.shape))
    transport.all_gather_rows(cand_all, cand)
    edges_p, edges_s = (merge or engine.time_pointers_merge)(cand_all, n_sta, n_t, k_tab, k_tab)
    return edges_p, edges_s, dt_partition


def exchange_halo_rows(rows_own, plan, n_sta, group=None, mode="a2a"):
    """Exchange of per-source-node row blocks: `rows_own` [n_own*S, C] -> halo rows [n_halo*S, C] in halo order: rank r sends, to
    every peer q, the S-row blocks of its owned nodes that q lists in `need[q][r]`. mode "a2a": one `all_to_all_single` with split
    sizes (RCCL on GPUs; gloo in the CPU tests); "p2p": one send / receive pair per peer, packed per destination
    (`Transport.halo_p2p_rows`)."""
    C = rows_own.shape[1]
    S = int(n_sta)
    blocks = rows_own.view(plan.n_own, S * C)
    recv = blocks.new_empty((plan.n_halo, S * C))
    if mode == "p2p":
        send = blocks.new_empty((int(sum(plan.send_counts)), S * C))
        if plan.world > 1:
            idx = [torch.as_tensor(x.astype(np.int64), device=rows_own.device) for x in plan.send_local]
            Transport(group, plan.world).halo_p2p_rows(recv, send, plan.recv_counts, plan.send_counts, plan.rank,
                                                       pack=lambda q, view: torch.index_select(blocks, 0, idx[q], out=view))
        return recv.view(plan.n_halo * S, C)
    send_idx = torch.as_tensor(np.concatenate(plan.send_local).astype(np.int64), device=rows_own.device)
    send = blocks.index_select(0, send_idx).contiguous() if send_idx.numel() else blocks.new_zeros((0, S * C))
    if plan.world > 1:
        Transport(group, plan.world).all_to_all_rows(recv, send, plan.recv_counts, plan.send_counts)
    return recv.view(plan.n_halo * S, C)


def gather_index(plan):
    """int64 [G]: position of global source node g inside the all-gathered `[world, n_max, C]` buffer."""
    n_max = max(len(o) for o in plan.owned)
    idx = np.empty(plan.n_grid, dtype=np.int64)
    for r in range(plan.world):
        idx[plan.owned[r]] = r * n_max + np.arange(len(plan.owned[r]))
    return idx, n_max


def allgather_owned(x_own, plan, group=None, index=None):
    """All-gather a per-owned-source-node tensor `[n_own, C]` into global order `[G, C]`: one collective on rows padded to
    the largest shard and one `index_select` with the precomputed `gather_index(plan)`."""
    if index is None:
        idx, n_max = gather_index(plan)
        index = (torch.as_tensor(idx, device=x_own.device), n_max)
    idx_t, n_max = index
    pad = x_own if plan.n_own == n_max else torch.cat((x_own, x_own.new_zeros((n_max - plan.n_own, x_own.shape[1]))))
    buf = x_own.new_empty((plan.world, n_max, x_own.shape[1]))
    Transport(group, plan.world).all_gather_rows(buf, pad.contiguous())
    return buf.view(-1, x_own.shape[1]).index_select(0, idx_t)


class ShardedPath(object):
    """Sharded DataAggregation + Bipartite on this rank's GPU, replicated SpatialAggregation / read-out.

    sta_csr: (rowptr, col) of the station graph; A_src_src: global [2, E]; pos_global: [G, 3]; pos_sta: optional [S, 3]
    station positions -> station processing order (the same on every rank: the halo rows of `wv` travel in that order).
    `overlap=False` runs the window as four sequential steps (stage 1, exchange, stage 2, all-gather) on one stream: the
    A/B reference for the overlapped schedule (bit-identical results).
    `subgraph` = dict(n_prod, sta_csr, src_csr, seg_rowptr) of the WHOLE irregular product graph (`use_subgraph`, as
    `engine.HipPath(subgraph=)` takes it): the shard is then over rows (`SubgraphShardPlan`: ragged halo, exchange counts in rows, the
    local context `genie_ctx_create_subgraph_ext`); `sta_csr` is ignored. The same schedules; the front and the replicated tail only
    (no association heads, no time-pointer tables, the default model definition)."""

    def __init__(self, n_sta, n_grid, sta_csr, A_src_src, pos_global, world, rank, device, group=None, scale_rel=30000.0,
                 pos_sta=None, overlap=True, halo="a2a", emulate=False, subgraph=None):
        self.group = group
        self.n_sta, self.n_grid = int(n_sta), int(n_grid)
        order = engine.sfc_order(np.asarray(pos_global))
        self.overlap = bool(overlap)
        if halo not in ("a2a", "p2p"):
            raise ValueError("halo must be 'a2a' (one all_to_all_single) or 'p2p' (one send / receive pair per peer)")
        self.halo = halo
        self.irregular = subgraph is not None
        if self.irregular:
            to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            self.plan = p = SubgraphShardPlan(to_np(subgraph["seg_rowptr"]), [to_np(t) for t in subgraph["src_csr"]],
                                              [to_np(t) for t in subgraph["sta_csr"]], n_grid, world, rank, order)
            if p.n_prod != int(subgraph["n_prod"]):
                raise ValueError("subgraph: seg_rowptr does not end at n_prod")
            if p.n_rows_own < 1:
                raise ValueError("rank %d of %d owns no product node of the irregular product graph" % (rank, world))
            self.n_prod = p.n_prod
            self.rows_own, self.rows_halo, self.rows_ext, self._unit = p.n_rows_own, p.n_rows_halo, p.n_rows_ext, 1
            t = torch.from_numpy
            self.local = engine.HipPath(n_sta, p.n_own, None, None, scale_rel=scale_rel, device=device, subgraph={
                "n_prod": p.n_rows_own, "n_prod_ext": p.n_rows_ext, "sta_csr": (t(p.sta_rowptr), t(p.sta_col)),
                "src_csr": (t(p.src_rowptr), t(p.src_col)), "seg_rowptr": t(p.seg_rowptr)})
            send = p.send_rows
        else:
            self.plan = p = ShardPlan(A_src_src, n_grid, world, rank, order)
            S = self.n_sta
            self.n_prod = self.n_grid * S
            # rows of the local lists; `_unit`: rows per exchanged block (a source node's S rows; one row on an irregular graph)
            self.rows_own, self.rows_halo, self.rows_ext, self._unit = p.n_own * S, p.n_halo * S, p.n_ext * S, S
            self.local = engine.HipPath(n_sta, p.n_own, sta_csr, (torch.from_numpy(p.src_rowptr), torch.from_numpy(p.src_col)),
                                        n_grid_ext=p.n_ext, grid_order=p.proc_order, scale_rel=scale_rel, device=device,
                                        sta_order=engine.sfc_order(np.asarray(pos_sta)) if pos_sta is not None else None)
            send = p.send_local
        self._send_blocks = send         # per peer: the local blocks (source nodes, or rows of an irregular graph) sent to it
        self.full = engine.HipPath(1, n_grid, (torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)),
                                   engine.csr_from_edges(torch.as_tensor(A_src_src), n_grid), grid_order=None,
                                   scale_rel=scale_rel, device=device)
        self.device = dev = self.local.device
        self.transport = Transport(group, world, emulate=emulate)
        S = self.n_sta
        pitch = int(self.local.lib.genie_ws_v_pitch(self.local.ctx))
        self._pitch = pitch
        # static exchange state: send-row index, send buffer, the halo part of `wv` inside the workspace (received in place)
        self._send_idx = torch.as_tensor(np.concatenate(send).astype(np.int64) if world > 1 else np.zeros(0, np.int64), device=dev)
        self._send_bufs = {}             # row width -> send buffer (wv: 16 floats; the association heads' q2: 32)
        nl = -np.ones(self.n_grid, dtype=np.int32)
        nl[p.own_global] = np.arange(p.n_own, dtype=np.int32)
        self.node_local = torch.as_tensor(nl, device=dev)          # global source node -> local owned index, -1 = owned elsewhere
        idx, n_max = gather_index(p)
        self._gather = (torch.as_tensor(idx, device=dev), n_max)
        self._bip_pad = torch.zeros((n_max, 15), dtype=torch.float32, device=dev)
        # irregular: the local context numbers its nodes in processing order; its [n_own, 15] output goes back to `own_global` order
        self._bip_unproc = torch.as_tensor(np.argsort(p.proc_order).astype(np.int64), device=dev) if self.irregular else None
        self.comm_stream = torch.cuda.Stream(device=dev) if self.local.device.type == "cuda" else None
        self.tail_stream = torch.cuda.Stream(device=dev) if self.local.device.type == "cuda" else None
        self._tail_done = None

    @property
    def contexts(self):
        """Both HIP contexts of the shard: the P-sized local one and the replicated G-sized one."""
        return (self.local, self.full)

    def set_weights(self, named):
        self.local.set_weights(named)
        self.full.set_weights(named)

    def sync_weights(self, params, view=None):
        """`HipPath.sync_weights` for both contexts (the P-sized shard and the replicated G-sized tail)."""
        self.local.sync_weights(params, view)
        self.full.sync_weights(params, view)

    def row_index(self, own_only=False):
        """int64 device tensor: the rows of a full `[G * S, C]` per-product-node tensor (p = g * S + s, process_utils.py:720-722)
        that make up this rank's local rows (owned + halo blocks, or the owned blocks only). Built once."""
        key = "_rows_own" if own_only else "_rows_ext"
        idx = getattr(self, key, None)
        if idx is None and self.irregular:      # the plan's global row ids as they are
            idx = torch.as_tensor(self.plan.own_rows if own_only else self.plan.ext_rows, dtype=torch.int64, device=self.device)
            setattr(self, key, idx)
        elif idx is None:
            g = torch.as_tensor(self.plan.own_global if own_only else self.plan.ext_global, dtype=torch.int64, device=self.device)
            idx = (g.view(-1, 1) * self.n_sta + torch.arange(self.n_sta, dtype=torch.int64, device=self.device).view(1, -1)).reshape(-1)
            setattr(self, key, idx)
        return idx

    def local_rows(self, t, name, cols, own_only=False):
        """This rank's rows of a per-product-node input: a `ShardRows` is taken as it is (its row count is checked), a full
        `[G * S, cols]` tensor (the reference's argument) is cut down by ONE `index_select` on the device it lives on."""
        n_loc = self.rows_own if own_only else self.rows_ext
        if isinstance(t, ShardRows):
            if t.own_only != own_only and self.rows_halo:
                if own_only and not t.own_only:           # owned blocks come first in the local order
                    return engine._f32(t.t, name, (self.rows_ext, cols))[:n_loc]
                raise ValueError("%s: rows of the owned source nodes only, the halo rows are needed too" % name)
            return engine._f32(t.t, name, (n_loc, cols))
        t = torch.as_tensor(t)
        if tuple(t.shape) != (self.n_prod, cols):
            raise ValueError("%s: expected shape (%d, %d) (all product nodes) or a ShardRows of %d local rows, got %s"
                             % (name, self.n_prod, cols, n_loc, tuple(t.shape)))
        idx = self.row_index(own_only)
        if t.device != idx.device:
            return t.index_select(0, idx.to(t.device)).to(self.device, torch.float32)
        return t.index_select(0, idx).float()

    def set_edge_features(self, pos_sta, pos_src_global):
        """`use_updated_model_definition` on the shard (genie_set_edge_features): the mean edge features of the owned source nodes
        come from the local CSR over the EXTENDED node list, so the positions of the halo nodes travel with the plan, not per window."""
        self._cartesian_only("set_edge_features (use_updated_model_definition)")
        ext = torch.as_tensor(self.plan.ext_global, dtype=torch.long)
        pos = torch.as_tensor(pos_src_global).float()
        self.local.set_edge_features(torch.as_tensor(pos_sta).float().to(self.device), pos[ext].contiguous().to(self.device))

    def set_absolute_pos(self, pos_sta, pos_src_global):
        """`use_absolute_pos` on the shard (genie_set_absolute_pos): scaled positions of the stations and of the extended node list."""
        self._cartesian_only("set_absolute_pos (use_absolute_pos)")
        ext = torch.as_tensor(self.plan.ext_global, dtype=torch.long)
        pos = torch.as_tensor(pos_src_global).float()
        self.local.set_absolute_pos(torch.as_tensor(pos_sta).float().to(self.device), pos[ext].contiguous().to(self.device))

    def _cartesian_only(self, what):
        if self.irregular:
            raise NotImplementedError("%s is not available on a source-node shard of an irregular product graph (use_subgraph): it serves "
                                      "the front and the replicated tail of the default model definition" % what)

    def set_subgraph_stations(self, sta_of_prod):
        """Station of every product node of the WHOLE irregular graph -> the local context's owned + halo rows (`embed_window`)."""
        if not self.irregular:
            raise ValueError("set_subgraph_stations: not an irregular product graph")
        t = torch.as_tensor(sta_of_prod).reshape(-1)
        if t.numel() != self.n_prod:
            raise ValueError("sta_of_prod must have n_prod entries")
        self.local.set_subgraph_stations(t.cpu()[torch.from_numpy(self.plan.ext_rows)])

    def wv_view(self):
        """Float view [local rows (owned, then halo), 16] of the projected operand `wv` inside the local workspace."""
        lp = self.local
        ptr = lp.lib.genie_ws_v_ptr(lp.ctx, lp._ws_ptr)
        off = int(ptr) - lp.ws.data_ptr()
        n = self.rows_ext * self._pitch
        return lp.ws[off: off + 4 * n].view(torch.float32).view(self.rows_ext, self._pitch)

    def _exchange(self, wv):
        """Pack the SEND rows, all-to-all, halo rows received in place (the halo part of `wv` is contiguous, grouped by owner). `wv`:
        any per-product-node operand [local rows, pitch] in the local row space (the workspace's wv rows, the association heads' q2).
        A block is the S rows of a source node; on an irregular graph one row (ragged counts: `SubgraphShardPlan`)."""
        p, S = self.plan, self._unit
        pitch = int(wv.shape[1])
        send_buf = self._send_bufs.get(pitch)
        if send_buf is None:
            send_buf = self._send_bufs[pitch] = torch.empty((int(self._send_idx.numel()), S * pitch), dtype=torch.float32, device=self.device)
        if p.world == 1 and not self.transport.on and not self.transport.emulate:
            return                      # no process group at all. (With one, EVERY rank enters the collective, also a rank with
                                        # nothing to exchange and the single rank of a world-size-1 group: the RCCL code path of the
                                        # 1-GPU tests and of `bench.py --gpus 1 --mode sharded`)
        blocks = wv[: self.rows_own].view(self.rows_own // S, S * pitch)
        recv = wv[self.rows_own:].view(self.rows_halo // S, S * pitch)
        if self.halo == "p2p":       # bucketed by destination: pack of peer q + 1 under the transfer of peer q, largest pair first
            if getattr(self, "_send_idx_q", None) is None:
                self._send_idx_q = [torch.as_tensor(x.astype(np.int64), device=self.device) for x in self._send_blocks]
            self.transport.halo_p2p_rows(recv, send_buf, p.recv_counts, p.send_counts, p.rank,
                                         pack=lambda q, view: torch.index_select(blocks, 0, self._send_idx_q[q], out=view))
            return
        if self._send_idx.numel():
            torch.index_select(blocks, 0, self._send_idx, out=send_buf)
        self.transport.all_to_all_rows(recv, send_buf, p.recv_counts, p.send_counts)

    def front(self, Slice_ext, Mask_ext, edge_attr_own, x_latent_out=None):
        """Sharded DataAggregation + Bipartite of one window on the current stream (+ the communication stream): returns this rank's
        Bipartite output `[n_own, 15]`, produced on the current stream. `x_latent_out` [n_own * S, 30]: the DataAggregation output of
        the owned rows is written there too (the association heads' input)."""
        p, S = self.plan, self.n_sta
        lp = self.local
        lp.check_input_range()         # (verdicts of the windows that have completed: engine.HipPath.check_input_range)
        P_ext = self.rows_ext
        Slice_ext = engine._f32(Slice_ext, "Slice", (P_ext, 4))
        Mask_ext = engine._f32(Mask_ext, "Mask", (P_ext, 4))
        edge_attr_own = engine._f32(edge_attr_own, "edge_attr", (self.rows_own, 3))
        ea = getattr(lp, "_static_ea", None)
        if ea is None or ea.data_ptr() != edge_attr_own.data_ptr() or edge_attr_own._version != lp._static_ea_version:
            # the static edge_attr of the owned rows: registered once, so that stage 2 reads its processing-order copy and runs
            # the straight-line row-layout kernel (k_stage2_ord) as the unsharded path does
            lp.set_static_edge_attr(edge_attr_own)
        Mask_own = Mask_ext[: self.rows_own]
        wv = self.wv_view()
        main = torch.cuda.current_stream(self.device)
        (s0, s1), (n0, n1), n = p.r_send, p.r_need, p.n_own
        if not self.overlap or (p.world == 1 and not self.transport.on and not self.transport.emulate):
            lp.da_stage1_range(Slice_ext, Mask_ext, 0, n, True)
            self._exchange(wv)
            lp.da_stage2_partials_range(Mask_own, edge_attr_own, 0, n, x_latent_out)
        else:
            comm = self.comm_stream
            lp.da_stage1_range(Slice_ext, Mask_ext, s0, s1, True)                 # rows other ranks wait for
            ev = torch.cuda.Event()
            ev.record(main)
            comm.wait_event(ev)
            with torch.cuda.stream(comm):
                self._exchange(wv)
                halo = torch.cuda.Event()
                halo.record(comm)
            lp.da_stage1_range(Slice_ext, Mask_ext, s1, n, False)                 # under the exchange
            lp.da_stage2_partials_range(Mask_own, edge_attr_own, 0, n0, x_latent_out)           # nodes without halo neighbours
            lp.da_stage2_partials_range(Mask_own, edge_attr_own, n1, n, x_latent_out)
            main.wait_event(halo)
            lp.da_stage2_partials_range(Mask_own, edge_attr_own, n0, n1, x_latent_out)
        bip_own = lp.bipartite_readout()
        return bip_own if self._bip_unproc is None else bip_own.index_select(0, self._bip_unproc)

    def gather_and_tail(self, bip_own, pos_global, tail=None):
        """All-gather of the Bipartite output, SpatialAggregation x3 (replicated) and `tail(x_spatial)` (the read-outs)."""
        p = self.plan
        idx_t, n_max = self._gather
        pad = self._bip_pad if p.n_own != n_max else None
        if pad is not None:
            pad[: p.n_own].copy_(bip_own)
        buf = bip_own.new_empty((p.world, n_max, 15))
        self.transport.all_gather_rows(buf, pad if pad is not None else bip_own)
        o = self.full.spatial_agg3(buf.view(-1, 15).index_select(0, idx_t), pos_global)
        return o if tail is None else tail(o)

    def assoc_fwd(self, y_latent, mask_src, x_latent_own, Mask_own, edge_attr_own):
        """The P-sized association heads on the shard (`HipPath.assoc_fwd_parts`): replicated y_latent [G, 30] / mask_src [G], this
        rank's x_latent / Mask / edge_attr rows -> s [n_own * S, 30]. Two halo exchanges on the current stream, one per layer: the q2
        rows (32 floats) before layer 1, the wv rows before the last pass -- the plan and transport of the DataAggregation window. Call
        after `front` of the same window."""
        self._cartesian_only("assoc_fwd (the association heads)")
        own = getattr(self, "_own_idx", None)
        if own is None:
            own = self._own_idx = torch.as_tensor(self.plan.own_global, dtype=torch.int64, device=self.device)
        y_own = engine._f32(y_latent, "y_latent", (self.n_grid, 30)).index_select(0, own)
        m_own = engine._f32(mask_src, "mask_src").reshape(-1).index_select(0, own)
        return self.local.assoc_fwd_parts(y_own, m_own, x_latent_own, Mask_own, edge_attr_own, self._exchange,
                                          lambda: self._exchange(self.wv_view()))

    def time_pointers(self, tlatent, max_t=None, dt=1.0, k=10, win=10.0):
        """The time-pointer tables of the whole product graph from this rank's own travel-time rows (`shard_time_pointers`: candidates
        per rank, one all-gather, merge on every rank). tlatent: a `ShardRows` of this rank's rows (owned, or owned + halo), or the whole [G * S, 2] table, of which only the owned rows are
        taken (cut out where the table lives). Returns (A_edges_p, A_edges_s, dt_partition, the owned rows as an own-only `ShardRows`)."""
        self._cartesian_only("time_pointers")
        tl_own = self.local_rows(tlatent, "tlatent", 2, own_only=True).contiguous()
        edges_p, edges_s, dt_partition = shard_time_pointers(tl_own, self.plan.own_global, self.n_sta, self.n_grid, self.transport,
                                                             max_t=max_t, dt=dt, k=k, win=win)
        return edges_p, edges_s, dt_partition, ShardRows(tl_own, own_only=True)

    def pick_rows(self, s_own, a_edges_p, a_edges_s, dt_partition, tpick, ipick, tlatent, timeout=60.0):
        """The rows of `s` and `tlatent` that the picks' time-pointer entries list, for both LocalSliceLgCollapse heads, from the
        ranks that own them: `HipPath.lslc_rows` on this rank's rows, ONE ragged all-gather of the compact lists, every row placed at
        its entry number -> table [2 * n_picks * 10, 32] (`HipPath.lslc_fwd_rows` takes it), the same on every rank. tlatent: the
        travel times of the whole product graph [G * S, >= 2], or a `ShardRows` of this rank's rows (tables built by `time_pointers`):
        either way the arrival of a listed row is read by its owner and travels in the row."""
        self._cartesian_only("pick_rows (the association heads)")
        own = isinstance(tlatent, ShardRows)
        if own:
            tlatent = self.local_rows(tlatent, "tlatent", int(tlatent.shape[1]), own_only=True)
        count, rows = self.local.lslc_rows(s_own, self.node_local, a_edges_p, a_edges_s, dt_partition, tpick, ipick, tlatent, tlatent_own=own)
        return place_pick_rows(self.transport.all_gather_ragged(rows, count, timeout), rows.shape[0])

    def path_fwd(self, Slice_ext, Mask_ext, edge_attr_own, pos_global, tail=None, pipelined=False):
        """Slice_ext / Mask_ext: [n_ext*S, 4] rows of owned then halo source nodes (local order). Returns x_spatial [G,30]
        (or `tail(x_spatial)`). `pipelined`: the all-gather and the G-sized kernels run on the tail stream, where they overlap
        the NEXT window's P-sized kernels (windows are independent in the apply loop); the result is then produced on
        `self.tail_stream` -- consume it there or after `wait_tail()`."""
        bip_own = self.front(Slice_ext, Mask_ext, edge_attr_own)
        if not pipelined:
            return self.gather_and_tail(bip_own, pos_global, tail)
        main = torch.cuda.current_stream(self.device)
        ev = torch.cuda.Event()
        ev.record(main)
        ts = self.tail_stream
        ts.wait_event(ev)
        bip_own.record_stream(ts)
        with torch.cuda.stream(ts):
            out = self.gather_and_tail(bip_own, pos_global, tail)
            self._tail_done = torch.cuda.Event()
            self._tail_done.record(ts)
        return out

    def wait_tail(self):
        if self._tail_done is not None:
            torch.cuda.current_stream(self.device).wait_event(self._tail_done)

