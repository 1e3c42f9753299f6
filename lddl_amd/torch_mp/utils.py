"""Rank / node helpers of lddl/torch_mp/utils.py: lddl_amd.torch's, with `get_dp_size`."""
from ..torch.utils import (barrier, get_dp_size, get_node_rank, get_nproc_per_node,  # noqa: F401
                           get_num_nodes, get_rank, get_world_size)
