"""The one reader of the package's RNNPOSE_* switches.  "0" means off, anything else (the empty string included) on.

Read when an engine / refiner is CONSTRUCTED (set the environment, then build a fresh PoseRefiner):
  name                      default  meaning                                                                     read in
  RNNPOSE_SPLIT_BATCH       1        update block: `parts` part-batch chains on their own streams                 UpdateEngine
  RNNPOSE_PARTS             2        ... how many; set explicitly: exactly that many, no small-batch merging      UpdateEngine
  RNNPOSE_SIDE_STREAM       0        flow-feature / flow-head side chain of a lone SMALL chain on a helper stream UpdateEngine
  RNNPOSE_FUSED_MASK        1        mask.2 inside the up-sampling kernel                                         UpdateEngine
  RNNPOSE_RESIDENT_1X1      1        convc1 / the encoder's output convolution in the LDS-resident 1x1 kernel     both engines
  RNNPOSE_FUSED_LOOKUP      0        window lookup + convc1 as ONE launch                                         UpdateEngine
  RNNPOSE_FUSED_INDUCED     0        pose-induced coordinates formed inside their first consumers                 UpdateEngine
  RNNPOSE_KSPLIT            1        small launches split their K loop (the engines pass a workspace)             both engines, ops (*)
  RNNPOSE_SPLIT_TENSORS     1        activations between convolutions as fp16 hi|lo split tensors                 UpdateEngine
  RNNPOSE_CONV_TILE         ""       tile shape per layer, "zr=3,q=1,heads=2" (0 auto; measurements)              UpdateEngine
  RNNPOSE_SPLIT_ENCODER     1        encoder: a single image batch in RNNPOSE_ENCODER_PARTS parts                 EncoderEngine
  RNNPOSE_ENCODER_PARTS     1        ... how many                                                                 EncoderEngine
  RNNPOSE_ENCODER_MERGE     unset    1 / 0: image sets always as one batch / always one stream each; unset: by size EncoderEngine
  RNNPOSE_SPLIT_FMAPS       1        the encoder writes the volume build's split operand format directly          PoseRefiner
  RNNPOSE_MIXED_PRECISION   0        one fp16 product per multiply-add, whatever cfg.raft.mixed_precision says    PoseRefiner

Read in every forward():
  RNNPOSE_FUSED_POSE        1        the outer pose update as one launch (ops.se3_outer_update)                   PoseRefiner.forward

Read when rnnpose_amd.ops is imported:
  RNNPOSE_RANGE_GUARD       1        the fp16x3 range guard counts clamped activation quads                       ops

Read ONCE per process, at the first convolution / LM step; unset leaves the library's own default untouched (nothing is called):
  RNNPOSE_SPATIAL_TILES     unset    0: row-major tiling of 3x3 layers                                            ops._apply_conv_env
  RNNPOSE_KSPLIT (*)        unset    0: launches never split K even when a workspace is passed                    ops._apply_conv_env
  RNNPOSE_LOOKUP_VARIANT    unset    0: the r01-r05 window-lookup kernel (bit-identical results)                  ops._apply_conv_env
  RNNPOSE_STRIP             unset    number, see ops.conv_strip (0: never the strip kernels)                      ops._apply_conv_env
  RNNPOSE_CORR_VARIANT      unset    0 / 1: volume kernel with register-staged / LDS-DMA operands                 ops._apply_conv_env
  RNNPOSE_KSPLIT_LIMITS     unset    "max_tiles,max_splits" (measurement)                                         ops._apply_conv_env
  RNNPOSE_LM_FUSED          unset    0 / 1: the three-launch / one-launch form of the LM step                     ops._apply_lm_env

What each one measured stands at the attribute it sets (UpdateEngine.__init__, EncoderEngine.__init__).  Not read through this module:
RNNPOSE_LIB (_lib.py: path of the library), RNNPOSE_HIPCC_EXTRA (build.py: compiler flags), RNNPOSE_DIST_BACKEND (distributed.py)."""
from __future__ import annotations

import os

text = os.environ.get        # text(name, default=None): the switch's string


def flag(name: str, default):
    """False for "0", True for anything else; `default` (which may be None: "leave it alone") when the switch is not set."""
    v = os.environ.get(name)
    return default if v is None else v != "0"


def number(name: str, default):
    """int of the switch; `default` when it is not set."""
    v = os.environ.get(name)
    return default if v is None else int(v)
