"""Allocator balance checks of the GPU tests: the library takes its device temporaries from
PyTorch's caching allocator (lddl_amd/context.py), so a block that a call fails to give back
shows in torch.cuda.memory_allocated()."""
import os

import pytest

# with LDDL_ARENA=own the library caches hipMalloc blocks of its own, which torch does not count
OWN_ARENA = os.environ.get('LDDL_ARENA') == 'own'
needs_torch_arena = pytest.mark.skipif(OWN_ARENA, reason='LDDL_ARENA=own: blocks are not torch\'s')


def allocated():
    """Bytes torch's allocator has handed out, once the device is idle."""
    import torch
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated()
