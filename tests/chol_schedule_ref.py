"""An independent reading of the ticket lists of the persistent Cholesky, written from the protocol table at the head of
slam-tricks_amd/csrc/chol_schedule.hpp and from nothing else of that header.

structure(...)  enumerates in numpy what the lists must contain: every task of the factorisation exactly once, every panel applied to
                every tile exactly once, one queue per tile row.
replay(...)     interprets the lists against integer flag arrays with W workgroups per queue that each hold one ticket, and returns the
                final flags and whether every task finished.  Flags only rise and a queue's drawn prefix only grows with its
                completions, so running whatever can run until nothing can decides liveness exactly: the outcome does not depend on
                the order the workgroups are visited in.  The kernel's pre-drawn ticket (a second ticket held while a short task
                runs) is not modelled: a workgroup here holds a ticket only while it waits or runs, which is the conservative side.

A task is a row {type | nb << 16, b, z, w} of an int32 array; list q holds rows [lstart[q], lstart[q + 1])."""
import numpy as np

D, T, TI, U, UQ, TU = range(6)
NTU = 10
TU10_WRITERS = (0, 2, 5, 9)         # the diagonal blocks (I, I) of the ten 2 x 2-tile blocks q = I (I + 1) / 2 + J


def fields(tasks):
    t = np.asarray(tasks, dtype=np.int64).reshape(-1, 4)
    return t[:, 0] & 0xff, np.maximum(1, (t[:, 0] >> 16) & 0xff), t[:, 1], t[:, 2], t[:, 3]


def task_row(tasks):
    """the tile row every task writes"""
    ty, _, b, z, _ = fields(tasks)
    return np.select([(ty == D) | (ty == TI), ty == TU, (ty == T) | (ty == U)], [b, b + 1, z], z >> 2)


def row_queues(tasks, lstart, nrow):
    """per tile row, the set of queues that hold a task writing it"""
    lstart = np.asarray(lstart)
    assert lstart[0] == 0 and lstart[-1] == len(tasks) and (np.diff(lstart) >= 0).all()
    queue = np.repeat(np.arange(len(lstart) - 1), np.diff(lstart))
    row = task_row(tasks)
    assert (row >= 0).all() and (row < nrow).all()
    return [set(queue[row == r].tolist()) for r in range(nrow)]


def structure(tasks, lstart, nblk, nwide):
    ty, nb, b, z, w = fields(tasks)
    nrow = nblk + 4 * nwide
    assert ((np.asarray(tasks).reshape(-1, 4)[:, 0] & ~0xff00ff) == 0).all() and (ty <= TU).all()
    assert ((nb == 1) | (ty == U)).all(), "only whole-tile updates are batched"
    assert (b >= 0).all() and (b < nblk).all()
    # ---- D and TI of every panel once
    for k in (D, TI):
        assert np.array_equal(np.sort(b[ty == k]), np.arange(nblk))
        assert (z[ty == k] == 0).all() and (w[ty == k] == 0).all()
    # ---- TU: per panel but the last, four siblings of form 2 or the ten blocks, the diagonal ones of form 1
    tu_panels = np.zeros(nblk, dtype=bool)
    for p in range(nblk):
        m = (ty == TU) & (b == p)
        if p == nblk - 1:
            assert not m.any()
            continue
        sib = sorted(zip(z[m].tolist(), w[m].tolist()))
        four = [(q, 2) for q in range(4)]
        ten = [(q, 1 if q in TU10_WRITERS else 0) for q in range(NTU)]
        assert sib == four or sib == ten, (p, sib)
        tu_panels[p] = True
    # ---- panel solves: every row i > b + 1 of every panel as one whole task or two halves; every virtual row over its span
    solves = np.zeros((nblk, nrow, 3), dtype=np.int64)
    m = ty == T
    assert (w[m] >= 0).all() and (w[m] <= 2).all() and (z[m] >= 0).all() and (z[m] < nrow).all()
    np.add.at(solves, (b[m], z[m], w[m]), 1)
    want_whole_or_halves = np.zeros((nblk, nrow), dtype=bool)
    for p in range(nblk):
        want_whole_or_halves[p, p + 2:nblk] = True
    want_virtual = np.zeros((nblk, nrow), dtype=bool)
    for p in range(4 * nwide):
        want_virtual[p + 1:4 * (p // 4) + 4, nblk + p] = True
    whole, halves = solves[:, :, 0] == 1, (solves[:, :, 1] == 1) & (solves[:, :, 2] == 1)
    none = solves.sum(axis=2) == 0
    assert (np.where(want_whole_or_halves, (whole & (solves.sum(axis=2) == 1)) | (halves & (solves.sum(axis=2) == 2)), True)).all()
    assert (np.where(want_virtual, whole & (solves.sum(axis=2) == 1), True)).all()
    assert none[~(want_whole_or_halves | want_virtual)].all()
    # ---- every tile (i, j <= i) receives every panel b < j once: counted per 32-row quarter of the tile
    got = np.zeros((nrow, nblk, nblk, 4), dtype=np.int64)             # [i][j][panel][quarter]
    m = ty == U
    assert (z[m] >= 0).all() and (z[m] < nrow).all() and (w[m] >= 0).all() and (w[m] < nblk).all() and (b[m] - nb[m] + 1 >= 0).all()
    for k in range(int(nb.max())):                                   # the k-th panel from the end of every batch that long
        mk = m & (nb > k)
        np.add.at(got, (z[mk], w[mk], b[mk] - k), 1)
    m = ty == UQ
    assert (z[m] >= 0).all() and ((z[m] >> 2) < nblk).all() and (w[m] >= 0).all() and (w[m] < nblk).all()
    np.add.at(got, (z[m] >> 2, w[m], b[m], z[m] & 3), 1)
    for p in np.flatnonzero(tu_panels):
        got[p + 1, p + 1, p, :] += 1                                 # the siblings of a panel, as one update of the next diagonal tile
    want = np.zeros_like(got)
    for i in range(nblk):
        for j in range(1, i + 1):
            want[i, j, :j, :] = 1
    for p in range(4 * nwide):
        for j in range(p + 1, 4 * (p // 4) + 4):
            want[nblk + p, j, p:j, :] = 1
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # ---- one writer XCD per tile row.  (TI(p) counts for row p: the tile it writes at the head of virtual row nblk + p is written
    # once and by nobody else.  The last virtual row of a wide block has no other tile, and so no task.)
    rq = row_queues(tasks, lstart, nrow)
    assert all(len(q) == 1 for q in rq[:nblk]) and all(len(q) <= 1 for q in rq[nblk:]), [(r, q) for r, q in enumerate(rq) if len(q) != 1][:5]


class OutOfOrder(AssertionError):
    pass


def replay(tasks, lstart, nblk, nwide, workers):
    """-> dict(done, finished, total, dflag, tflag, ver); raises OutOfOrder if an update starts on a tile version that is not its own"""
    nrow = nblk + 4 * nwide
    tl = np.asarray(tasks, dtype=np.int64).reshape(-1, 4).tolist()
    dflag, loaded, tudone = [0] * nblk, [0] * nblk, [0] * nblk
    tflag = [[0] * nrow for _ in range(nblk)]          # [panel][row]
    ver = [[0] * nblk for _ in range(nrow)]            # [row][panel]
    nq = len(lstart) - 1
    nxt = [int(v) for v in lstart[:-1]]
    end = [int(v) for v in lstart[1:]]
    held = [[] for _ in range(nq)]                     # per queue: [ticket, stage] of every workgroup that holds one
    finished = 0

    def advance(e):
        """run the held ticket as far as the flags allow; True: the task is finished and published"""
        x, b, z, w = tl[e[0]]
        ty = x & 0xff
        if ty == D:
            if ver[b][b] < 4 * b:
                return False
            dflag[b] += 1
            return True
        if ty == TI:
            if dflag[b] < 1:
                return False
            if b < 4 * nwide:
                tflag[b][nblk + b] += 4
            return True
        if ty == T:
            if dflag[b] < 1 or ver[z][b] < 4 * (b - max(0, z - nblk)):
                return False
            tflag[b][z] += 4 if w == 0 else 2
            return True
        if ty == TU:
            if e[1] == 0:                               # parked on the ticket
                if ver[b + 1][b] < 4 * b or ver[b + 1][b + 1] < 4 * b:
                    return False
                e[1] = 1
            if e[1] == 1:                               # inside the task: the diagonal block, then its copy of the block row
                if dflag[b] < 1:
                    return False
                loaded[b] += 1
                if w == 2:
                    ver[b + 1][b + 1] += 1
                else:
                    tudone[b] += 1
                    if tudone[b] == NTU:
                        ver[b + 1][b + 1] += 4
                    if w == 0:
                        return True
                e[1] = 2
            if loaded[b] < (4 if w == 2 else NTU):      # the blocks that write X wait for every sibling's copy
                return False
            tflag[b][b + 1] += 1
            return True
        i = z >> 2 if ty == UQ else z
        nb = max(1, (x >> 16) & 0xff) if ty == U else 1
        if tflag[b][i] < 4 or tflag[b][w] < 4:
            return False
        waits_for = 4 * (b - nb + 1 - max(0, i - nblk))
        if ver[i][w] < waits_for:
            return False
        if ver[i][w] > waits_for + (3 if ty == UQ else 0):
            raise OutOfOrder("task %r starts on version %d of its tile, it waits for %d" % (tl[e[0]], ver[i][w], waits_for))
        ver[i][w] += 4 * nb if ty == U else 1
        return True

    progress = True
    while progress:
        progress = False
        for q in range(nq):
            h = held[q]
            while len(h) < workers and nxt[q] < end[q]:
                h.append([nxt[q], 0])
                nxt[q] += 1
            k = 0
            while k < len(h):
                stage = h[k][1]
                if advance(h[k]):
                    finished += 1
                    progress = True
                    if nxt[q] < end[q]:                 # the workgroup draws its next ticket and looks at it at once
                        h[k] = [nxt[q], 0]
                        nxt[q] += 1
                    else:
                        h.pop(k)
                else:
                    progress = progress or h[k][1] != stage
                    k += 1
    return dict(done=finished == len(tl), finished=finished, total=len(tl), dflag=np.array(dflag), tflag=np.array(tflag).reshape(nblk, nrow),
                ver=np.array(ver).reshape(nrow, nblk))


def check_final(r, nblk, nwide):
    """the counters at the end of a complete factorisation"""
    nrow = nblk + 4 * nwide
    assert (r["dflag"] == 1).all()
    ver_want = np.zeros((nrow, nblk), dtype=np.int64)
    tflag_want = np.zeros((nblk, nrow), dtype=np.int64)
    for i in range(nblk):
        ver_want[i, :i + 1] = 4 * np.arange(i + 1)
        tflag_want[:i, i] = 4
    for p in range(4 * nwide):
        span = np.arange(p, 4 * (p // 4) + 4)
        ver_want[nblk + p, span] = 4 * (span - p)
        tflag_want[span, nblk + p] = 4
    assert np.array_equal(r["ver"], ver_want), np.argwhere(r["ver"] != ver_want)[:5]
    assert np.array_equal(r["tflag"], tflag_want), np.argwhere(r["tflag"] != tflag_want)[:5]
