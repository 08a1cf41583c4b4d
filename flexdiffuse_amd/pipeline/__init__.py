from .flex import FlexPipeline  # noqa: F401
from .guide import GuideBase, PromptGuide, ScheduledGuide, SimpleGuide, WindowedGuide  # noqa: F401
