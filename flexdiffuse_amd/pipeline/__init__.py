from .flex import FlexPipeline  # noqa: F401
from .guide import GuideBase, PromptGuide, ScheduledGuide, SimpleGuide  # noqa: F401
