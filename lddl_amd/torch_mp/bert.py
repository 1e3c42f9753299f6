"""BERT pretraining loader for model-parallel training — drop-in for lddl/torch_mp/bert.py.

The reference copies lddl/torch and changes three things; here they are parameters of the shared
code (lddl_amd/torch):

* files are strided and DataLoader workers seeded by `dp_rank`, not by global rank
  (`ParquetDataset(dp_rank=...)`), so the ranks of one data-parallel group read the same
  samples in the same order;
* a static-masking batch also yields `masked_lm_positions`: despite the name the [B, L] int64
  loss mask, 1 at the sample's masked positions (lddl/torch_mp/bert.py:103-105, 150). The
  collate kernel writes it in its one output pass (lddl_collate_encode_mp);
* `get_bert_pretrain_data_loader` takes `dp_rank`.

Dynamic masking: the Philox key is `mask_seed(base_seed, dp_rank, bin_id)`, so all ranks of a
group apply the same mask to the same batch and different groups draw independent streams. The
reference masks with each worker's torch RNG and gets this only where the training script seeds
torch alike on those ranks; here it holds by construction.
"""
import logging

from ..torch import bert as _bert
from ..torch.bert import PackedBatch, _mask_tokens, encode_packed, mask_seed  # noqa: F401
from ..torch.dataloader import DataLoader


def _to_encoded_inputs(batch, tokenizer, sequence_length_alignment=8, ignore_index=-1):
    """lddl/torch_mp/bert.py:69-153. `tokenizer` is a lddl_amd.context.Context."""
    if len(batch[0]) > 3:
        assert len(batch[0]) == 5
    return encode_packed(PackedBatch(batch), tokenizer, sequence_length_alignment, ignore_index,
                         loss_mask=True)


def get_bert_pretrain_data_loader(path, local_rank=0, dp_rank=0, shuffle_buffer_size=16384,
                                  shuffle_buffer_warmup_factor=16, tokenizer_class=None,
                                  vocab_file=None, tokenizer_kwargs={}, data_loader_class=DataLoader,
                                  data_loader_kwargs={}, mlm_probability=0.15, base_seed=12345,
                                  log_dir=None, log_level=logging.INFO, return_raw_samples=False,
                                  start_epoch=0, sequence_length_alignment=8, ignore_index=-1,
                                  whole_word_masking=False):
    """Same arguments and yielded dicts as
    lddl.torch_mp.get_bert_pretrain_data_loader (lddl/torch_mp/bert.py:213-429); the tensors are
    on the current cuda device. dp_rank is this process's data-parallel rank, e.g. Megatron's
    `mpu.get_data_parallel_rank()`; the number of groups is max(dp_rank) + 1 over the world.
    whole_word_masking: as in lddl_amd.torch (one keyword past the reference's signature); the
    key is still the dp_rank group's, so the ranks of a group still yield identical batches."""
    assert isinstance(dp_rank, int) and dp_rank >= 0
    return _bert._bert_pretrain_data_loader(
        path, local_rank, dp_rank, shuffle_buffer_size, shuffle_buffer_warmup_factor,
        tokenizer_class, vocab_file, tokenizer_kwargs, data_loader_class, data_loader_kwargs,
        mlm_probability, base_seed, log_dir, log_level, return_raw_samples, start_epoch,
        sequence_length_alignment, ignore_index, whole_word_masking)
