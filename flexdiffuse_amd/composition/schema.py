'''Data contract of region-composited guidance.

Field names, order and defaults are those of the reference's composition/schema.py:6-26
(`Runner.compose` builds these from table rows, utils.py:188-201, and `CompositeGuide`
reads them); positions and sizes are in IMAGE pixels and are floor-divided by 8 into latent
blocks by the guide.
'''
from __future__ import annotations

import dataclasses
import json
from typing import Any, List, Tuple

import numpy as np

Pixels = Tuple[int, int]


def _as_mask(mask: Any, size: Pixels) -> np.ndarray:
    '''A soft mask over the box: 2-D array-like of floats in [0, 1], or a PIL image read as
    convert('L') / 255; shape (height, width) of the box in image pixels -> float32 array.'''
    try:
        from PIL import Image
    except ImportError:          # pragma: no cover -- PIL is optional for array masks
        Image = None
    if Image is not None and isinstance(mask, Image.Image):
        m = np.asarray(mask.convert('L'), dtype=np.float32) / np.float32(255)
    else:
        if hasattr(mask, 'detach'):
            mask = mask.detach().cpu().numpy()
        m = np.array(mask, dtype=np.float32)
    want = (int(size[1]), int(size[0]))
    if m.ndim != 2 or m.shape != want:
        raise ValueError(f'mask shape {m.shape} != the box (height, width) {want} in image pixels')
    if np.isnan(m).any():
        raise ValueError('mask holds NaN')
    if m.size and (m.min() < 0.0 or m.max() > 1.0):
        raise ValueError(f'mask values must lie in [0, 1], got [{m.min()}, {m.max()}]')
    return np.ascontiguousarray(m)


@dataclasses.dataclass
class EntitySchema():
    '''One prompt painted into a rectangle of the canvas.'''
    prompt: str
    offset: Pixels               # (x, y) of the box's top-left corner
    size: Pixels                 # (width, height) of the box
    blend: float = 0.8           # 0 = background only ... 1 = entity only, inside the box
    # optional soft shape inside the box (beyond the reference, whose schema leaves it as a TODO):
    # (height, width) weights in [0, 1] over the box's image pixels; None = the whole rectangle
    mask: Any = dataclasses.field(default=None, compare=False)

    def __post_init__(self):
        if len(self.offset) != 2 or len(self.size) != 2:
            raise ValueError('offset and size are (x, y) / (width, height) pairs')
        if self.mask is not None:
            self.mask = _as_mask(self.mask, self.size)


@dataclasses.dataclass
class Schema():
    '''A background prompt, two style prompts with their blend range, and the entities.'''
    background_prompt: str
    style_start_prompt: str
    style_end_prompt: str
    style_blend: Tuple[float, float]
    entities: List[EntitySchema]

    def json(self) -> str:
        '''Same JSON shape as the reference's `Schema.json()` (entities as plain dicts); an entity
        with a mask adds it as a nested list, one without adds nothing.'''
        d = dataclasses.asdict(self)
        for e, src in zip(d['entities'], self.entities):
            if src.mask is None:
                del e['mask']
            else:
                e['mask'] = src.mask.tolist()
        return json.dumps(d)
