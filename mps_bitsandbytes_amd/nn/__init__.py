"""
Quantized layers of the MI355X backend.

Each layer keeps the reference's public surface (mps_bitsandbytes/nn/*.py) and runs its forward through one entry
point of the HIP library: Linear4bit -> matmul_4bit, Linear8bit -> linear_int8, LinearFP8 -> matmul_fp8_e4m3, OutlierAwareLinear -> outlier_linear,
Embedding4bit / Embedding8bit -> embedding_4bit / embedding_8bit,
SwitchBackLinear -> switchback_linear (libmbnb_train.so), Linear4bitGroup (Linear4bit layers that share their input) ->
matmul_4bit_grouped (libmbnb_group.so), Linear4bitLoRA / Linear4bitLoRAGroup (a Linear4bit base with un-merged LoRA adapters) ->
matmul_4bit_lora_grouped (libmbnb_lora.so), Linear4bitMultiLoRA / Linear4bitMultiLoRAGroup (a bank of adapters, one chosen per row) ->
matmul_4bit_multilora_grouped (libmbnb_mlora.so), LinearMXFP4 (an OCP MXFP4 weight on the block-scaled MFMA) -> matmul_mxfp4
(libmbnb_mx.so), ExpertsMXFP4 (the MXFP4 expert weights of a mixture-of-experts projection, the expert of every (token, slot) pair
read on the device) -> matmul_mxfp4_experts (libmbnb_moe.so), MoEMLPMXFP4 (the gate / up and down expert weights of a gpt-oss MLP under
the checkpoint's names) -> moe_mlp_mxfp4 (libmbnb_moemlp.so), MoERouterTopK (the router of that block: logits, top-k and softmax in one
launch) -> moe_router_topk (libmbnb_router.so), MoEBlockMXFP4 (the router and the expert MLP under the checkpoint's `mlp.*` names) ->
moe_block_mxfp4.  `_base.py` holds what they share.
"""
from .embedding import Embedding4bit, Embedding8bit, EmbeddingFP4, EmbeddingNF4
from .linear4bit import Linear4bit, Params4bit
from .linear4bit_group import Linear4bitGroup
from .linear4bit_lora import Linear4bitLoRA, Linear4bitLoRAGroup
from .linear4bit_multilora import Linear4bitMultiLoRA, Linear4bitMultiLoRAGroup
from .linear8bit import Linear8bit
from .linear_fp8 import LinearFP8
from .linear_mxfp4 import LinearMXFP4
from .experts_mxfp4 import ExpertsMXFP4
from .moe_mlp_mxfp4 import MoEMLPMXFP4
from .moe_block_mxfp4 import MoEBlockMXFP4, MoERouterTopK
from .outlier_aware import OutlierAwareLinear
from .switchback import SwitchBackLinear, SwitchBackLinearCallback

__all__ = sorted(['Linear4bit', 'Linear4bitGroup', 'Linear4bitLoRA', 'Linear4bitLoRAGroup', 'Linear4bitMultiLoRA', 'Linear4bitMultiLoRAGroup', 'Params4bit', 'Linear8bit', 'LinearFP8', 'LinearMXFP4', 'ExpertsMXFP4', 'MoEMLPMXFP4', 'MoERouterTopK', 'MoEBlockMXFP4', 'OutlierAwareLinear',
                  'Embedding4bit', 'Embedding8bit', 'EmbeddingNF4', 'EmbeddingFP4',
                  'SwitchBackLinear', 'SwitchBackLinearCallback'])
