from .guide import CompositeGuide, WindowedCompositeGuide  # noqa: F401
from .schema import EntitySchema, Schema  # noqa: F401
