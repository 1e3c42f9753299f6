"""Compact MLM targets on the device (past the reference): the masked slots of a
batch's dense `labels` as fixed-shape tensors, for a training step that runs the MLM head only
on them.

    labels [R, L] --compact_labels (lddl_mlm_compact_rows / lddl_mlm_compact_flat)-->
      rows: masked_lm_positions, masked_lm_ids, masked_lm_weights [R, P], num_masked [R]
      flat: masked_lm_flat_positions, masked_lm_flat_ids [R * P], num_masked [R],
            num_masked_total [1]

`labels.view(-1) != ignore_index` followed by `nonzero()` yields the same positions, but waits
for the host and returns a shape that changes from step to step. Here every shape is known on
the host, nothing waits for the GPU and nothing depends on the data, so the call is safe in a
captured training step. `CompactMLMTargets` is the same as the `collate_fn` of every loader.
Importing this module loads neither torch nor the native library."""


LAYOUTS = ('rows', 'flat')


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def _validate(max_predictions_per_seq, layout, ignore_index):
    if not _is_int(max_predictions_per_seq) or max_predictions_per_seq < 1:
        raise ValueError('max_predictions_per_seq must be an int >= 1, not {!r}'.format(
            max_predictions_per_seq))
    if layout not in LAYOUTS:
        raise ValueError("layout must be 'rows' or 'flat', not {!r}".format(layout))
    if not _is_int(ignore_index) or not -(1 << 63) <= ignore_index < (1 << 63):
        raise ValueError('ignore_index must be an int (64-bit), not {!r}'.format(ignore_index))


def compact_labels(labels, max_predictions_per_seq, ignore_index=-1, layout='rows'):
    """The masked slots (label != ignore_index) of `labels`, a cuda int64 [R, L] tensor, in
    position order, as a dict of fixed-shape tensors on its device. P = max_predictions_per_seq.

    layout='rows': per row r with n_r masked slots x_0 < x_1 < ..., k = min(n_r, P):
      masked_lm_positions [R, P] int64   x_j for j < k, then 0
      masked_lm_ids       [R, P] int64   labels[r, x_j] for j < k, then ignore_index
      masked_lm_weights   [R, P] float32 1 for j < k, then 0
      num_masked          [R]    int32   n_r, the true count
    layout='flat': the same over labels.view(-1), with capacity R * P:
      masked_lm_flat_positions [R * P] int64  the indices r * L + x ascending, then 0
      masked_lm_flat_ids       [R * P] int64  their labels, then ignore_index
      num_masked               [R]     int32  n_r
      num_masked_total         [1]     int64  the sum of n_r

    Overflow: a row with n_r > P (flat: a batch with more than R * P masked slots) keeps the
    first P (R * P) in position order and drops the rest; num_masked (num_masked_total) still
    holds the true count, so the consumer can see it without this call deciding anything.

    Runs on the current stream of labels' device: the outputs are torch.empty, one launch
    (flat: two) writes every element of them, and nothing waits for the GPU. A non-contiguous
    view is made contiguous first."""
    _validate(max_predictions_per_seq, layout, ignore_index)
    import torch
    from .._native import check, lib
    from ..context import _ptr
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int64
            and labels.dim() == 2):
        raise ValueError('labels must be a cuda int64 [R, L] tensor')
    labels = labels.contiguous()
    R, L = labels.shape
    P = max_predictions_per_seq
    dev = labels.device
    num = torch.empty(R, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if layout == 'rows':
            pos = torch.empty(R, P, dtype=torch.int64, device=dev)
            ids = torch.empty(R, P, dtype=torch.int64, device=dev)
            w = torch.empty(R, P, dtype=torch.float32, device=dev)
            if R:  # (no rows: nothing to write, and an empty tensor has no pointer to pass)
                check(lib.lddl_mlm_compact_rows(stream, _ptr(labels), R, L, ignore_index, P,
                                                _ptr(pos), _ptr(ids), _ptr(w), _ptr(num)))
            return {'masked_lm_positions': pos, 'masked_lm_ids': ids, 'masked_lm_weights': w,
                    'num_masked': num}
        cap = R * P
        pos = torch.empty(cap, dtype=torch.int64, device=dev)
        ids = torch.empty(cap, dtype=torch.int64, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        if R:
            check(lib.lddl_mlm_compact_flat(stream, _ptr(labels), R, L, ignore_index, cap,
                                            _ptr(pos), _ptr(ids), _ptr(num), _ptr(total)))
        else:  # capacity 0: the entry point takes none below 1, and only the total is left
            total.zero_()
    return {'masked_lm_flat_positions': pos, 'masked_lm_flat_ids': ids, 'num_masked': num,
            'num_masked_total': total}


class CompactMLMTargets:
    """A `collate_fn` that adds `compact_labels(batch['labels'], ...)` to every batch dict.

    It plugs into the hook every loader already has: `data_loader_kwargs={'collate_fn': hook}`
    of get_bert_pretrain_data_loader, get_bert_pretrain_packed_data_loader and
    torch_mp.get_bert_pretrain_data_loader (applied in the main process to the encoded batch, on
    the device), `collate_fn=hook` of the online loaders.

      max_predictions_per_seq  P, an int >= 1: slots per row ('rows'), R * P in all ('flat')
      layout                   'rows' or 'flat' (see compact_labels for the keys of each)
      ignore_index             MUST be the loader's ignore_index (default -1 on both sides): the
                               hook sees only the batch and cannot read the loader's own value
      keep_labels              False drops the dense `labels` from the batch
      then                     called with the batch afterwards; its result is returned

    Sizing P: with dynamic masking a row's count is binomial(m, mlm_probability) over its m
    non-special slots: mean m p, variance m p (1 - p). At L = 512, p = 0.15: mean <= 76.4,
    sigma <= 8.1, so P = 128 is more than six sigma away; P = ceil(L p + 6 sqrt(L p (1 - p)))
    is a safe rule, and the flat form needs only the mean of a batch plus its much smaller
    spread. Static masks hold at most the preprocessor's max_predictions_per_seq. On overflow
    the first P slots (R * P) in position order are kept and num_masked tells the true count.

    The packed loaders put several samples into one row of max_seq_length slots, so there P
    counts per ROW, not per sample: size it for max_seq_length, or better use layout='flat',
    whose one capacity serves the batch whatever the rows hold.

    torch_mp's static-masking batches already hold a `masked_lm_positions`: despite the name the
    dense [B, L] loss mask. With layout='rows', whose positions take that name, the loss mask
    stays in the batch as `loss_mask`; with 'flat' nothing collides and it keeps its name. Any
    other key that is already there raises ValueError.

    A batch without `labels` (return_raw_samples=True, whose hook gets the raw samples; or
    collate_pairs without a mask on a table without static masks, which yields
    special_tokens_mask instead) raises KeyError."""

    def __init__(self, max_predictions_per_seq, layout='rows', ignore_index=-1, keep_labels=True,
                 then=None):
        _validate(max_predictions_per_seq, layout, ignore_index)
        if then is not None and not callable(then):
            raise ValueError('then must be callable or None')
        self.max_predictions_per_seq = max_predictions_per_seq
        self.layout = layout
        self.ignore_index = ignore_index
        self.keep_labels = bool(keep_labels)
        self.then = then

    def __call__(self, batch):
        if not isinstance(batch, dict) or 'labels' not in batch:
            raise KeyError(
                "CompactMLMTargets: the batch has no 'labels' ({}): the hook needs an encoded "
                'batch with MLM labels, not raw samples (return_raw_samples=True) and not the '
                "online collate's plain form without masking (special_tokens_mask)".format(
                    'keys ' + ', '.join(map(str, batch)) if isinstance(batch, dict)
                    else type(batch).__name__))
        new = compact_labels(batch['labels'], self.max_predictions_per_seq, self.ignore_index,
                             self.layout)
        for k in new:
            if k not in batch:
                continue
            if k == 'masked_lm_positions' and 'loss_mask' not in batch:
                batch['loss_mask'] = batch[k]  # torch_mp's dense [B, L] mask under its own name
            else:
                raise ValueError('CompactMLMTargets: the batch already has {!r}'.format(k))
        batch.update(new)
        if not self.keep_labels:
            del batch['labels']
        return self.then(batch) if self.then is not None else batch
