"""Worker-side half of the sequence-packing BERT loader: the row plan of a batch and
the `PackedBatch` that carries it.

Several samples share one row of `capacity` (= max_seq_length) slots. The DataLoader workers know
every sample's token counts, so the plan is made here, on the host, and the process that owns the
GPU never waits for a shape. Like `packing`, this module imports neither the native library nor
anything that touches the GPU."""
import functools
import time
from collections import namedtuple

import numpy as np

from .packing import PackedBatch

# row, start, seq_in_row, fill: per sample, in the batch's order; order: the samples sorted by
# (row, start); R: number of rows; capacity: slots per row
SeqPlan = namedtuple('SeqPlan', 'row start seq_in_row fill order R capacity')


def plan_rows(lengths, capacity):
    """First-fit decreasing: samples are visited by length descending (ties: the lower index
    first), each goes into the lowest-numbered open row with at least its length free, else
    into a new row; inside a row samples sit back to back in the order they were placed.

    lengths[i] = na[i] + nb[i] + 3. Returns a SeqPlan. `seq_in_row` is 1-based. `fill[i]` is the
    number of slots sample i's wave writes: its length, plus the row's unused tail if it is the
    last sample of its row, so the fill regions tile the [R, capacity] outputs exactly once."""
    lengths = np.asarray(lengths, np.int64)
    B = len(lengths)
    capacity = int(capacity)
    if B and int(lengths.max()) > capacity:
        raise ValueError('a sample of length {} does not fit a row of capacity {}'.format(
            int(lengths.max()), capacity))
    row = np.zeros(B, np.int32)
    start = np.zeros(B, np.int32)
    seq = np.zeros(B, np.int32)
    fill = lengths.astype(np.int32)
    free = np.full(B, capacity, np.int64)  # free[r] of the open rows r < R
    count = np.zeros(B, np.int32)
    last = np.zeros(B, np.int64)           # the sample placed last into row r
    R = 0
    for i in np.argsort(-lengths, kind='stable'):
        n = lengths[i]
        fits = free[:R] >= n
        r = int(fits.argmax()) if fits.any() else R
        R = max(R, r + 1)
        row[i] = r
        start[i] = capacity - free[r]
        count[r] += 1
        seq[i] = count[r]
        free[r] -= n
        last[r] = i
    fill[last[:R]] += free[:R].astype(np.int32)
    order = np.lexsort((start, row)).astype(np.int64)
    return SeqPlan(row, start, seq, fill, order, R, capacity)


class SeqPackedBatch(PackedBatch):
    """A PackedBatch with the row plan of its samples (built in a DataLoader worker, picklable)."""

    def __init__(self, batch, max_seq_length):
        super().__init__(batch)
        t0 = time.perf_counter()
        self.plan = plan_rows(self.na.astype(np.int64) + self.nb + 3, max_seq_length)
        self.pack_s += time.perf_counter() - t0


def _seqpack_batch(batch, max_seq_length):
    return SeqPackedBatch(batch, max_seq_length)


def seqpack_collate(max_seq_length):
    """The DataLoader collate_fn of the packing loader (a picklable partial of a module-level
    function, next to packing._pack_batch)."""
    return functools.partial(_seqpack_batch, max_seq_length=max_seq_length)
