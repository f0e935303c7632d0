from .block import LORA_FFN_TARGETS, LORA_TARGETS, MI355XWanBlock, WanBlockLayout  # noqa: F401
from .control_specification import MI355XWanControlModelSpecification, MI355XWanControlSpecOps  # noqa: F401
from .fsdp import ParameterSharder  # noqa: F401
from .model import MI355XWanTransformer3DModel, WanTransformerConfig, rotary_tables  # noqa: F401
from .sampler import MI355XWanLatentSampler, wan_flow_match_sigmas, wan_unipc_schedule, wan_unipc_tables  # noqa: F401
from .specification import MI355XWanModelSpecification, MI355XWanSpecOps  # noqa: F401
from .trainer import MI355XWanFullFinetuneStep, MI355XWanLoRAStep  # noqa: F401
