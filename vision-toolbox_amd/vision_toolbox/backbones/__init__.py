"""Backbones of the MI355X hot path: Darknet / CSPDarknet / DarknetYOLOv5 / VoVNet / ConvNeXt / MLP-Mixer / ViT / Swin / CaiT /
PatchConvNet / DeiT / ResNet / RegNet / MobileNet / EfficientNet.

Both surfaces the reference snapshot exposes are exported: the classes with
`from_config` (reference backbones/__init__.py:3,10, tests/test_backbones.py:25-30) and the
named factories that classifier.py:58 / README.md:27 / the checkpoint file names use.
ConvNeXt (V1 on the GPU; V2's GlobalResponseNorm on CPU tensors only) is exported as the class with
`from_config`, as the reference does (backbones/convnext.py:112), and so is MLPMixer (backbones/mlp_mixer.py:39), the
first family without convolutions: its token mixing runs on the transposed-GEMM kernels of vt_token_mix.hip.  ViT
(backbones/vit.py:111, with its blocks MHA / ViTBlock / MHAPooling) runs on the fused attention kernels of vt_attention.hip,
and SwinTransformer (backbones/swin.py:127, with WindowAttention / SwinBlock / PatchMerging), the hierarchical one, on the
shifted-window kernels of vt_window_attention.hip.  CaiT (backbones/cait.py:101, with ClassAttention / TalkingHeadAttention /
CaiTCABlock / CaiTSABlock) runs its talking-heads and class attention on the kernels of vt_talking_attention.hip.
PatchConvNet (backbones/patchconvnet.py:106, with PatchConvBlockLN / PatchConvBlockBN / AttentionPooling and a
SqueezeExcitation of our own: torchvision is not imported) runs on the plane, gate and pooling kernels of vt_patchconv.hip.
DeiT and DeiT3 (backbones/deit.py:14,118), the other family the reference builds on ViT, run on ViT's block path; DeiT's
two prefix tokens and its two-token pooled head run on the kernels of vt_prefix_tokens.hip.  ResNetExtractor
(backbones/torchvision_models.py:22, with BasicBlock / Bottleneck written out under torchvision's child names: torchvision
is not imported) runs its add-then-ReLU block ends and its 7x7 stem on the kernels of vt_resnet.hip.  RegNetExtractor
(the next class of that file, RegNetBlock written out the same way) runs its grouped 3x3 convolutions in one launch per pass
and its Squeeze-Excitation MLP on the kernels of vt_gconv.hip.  MobileNetExtractor (the class after it: mobilenet_v2,
mobilenet_v3_large, mobilenet_v3_small, InvertedResidual written out the same way) runs its depthwise Conv-BN-act units on the
tiled kernels of vt_dwtile.hip, with ReLU6 / Hardswish in the BatchNorm passes and the hardsigmoid gate of VoVNet's eSE.
EfficientNetExtractor (the last class of that file: efficientnet_b0 .. b7 and efficientnet_v2_s / m / l, MBConv / FusedMBConv
written out the same way) adds training-mode stochastic depth -- a per-image keep factor in the BatchNorm passes that close
a residual block -- and the Squeeze-Excitation pool inside the depthwise unit's normalise pass (vt_mbconv.hip).
"""
from .base import BaseBackbone
from .convnext import ConvNeXt, ConvNeXtBlock, GlobalResponseNorm
from .mlp_mixer import MLP, MixerBlock, MLPMixer
from .vit import MHA, MHAPooling, ViT, ViTBlock
from .deit import DeiT, DeiT3
from .cait import CaiT, CaiTCABlock, CaiTSABlock, ClassAttention, TalkingHeadAttention
from .patchconvnet import AttentionPooling, PatchConvBlockBN, PatchConvBlockLN, PatchConvNet, SqueezeExcitation
from .swin import PatchMerging, SwinBlock, SwinTransformer, WindowAttention, window_partition, window_unpartition
from .resnet import BasicBlock, Bottleneck, ResNetExtractor
from .regnet import RegNetBlock, RegNetExtractor, regnet_block_params
from .mobilenet import InvertedResidualV2, InvertedResidualV3, MobileNetExtractor
from .efficientnet import EfficientNetExtractor, FusedMBConv, MBConv
from .darknet import (
    CSPDarknetStage,
    Darknet,
    DarknetBlock,
    DarknetStage,
    DarknetYOLOv5,
    cspdarknet53,
    darknet19,
    darknet53,
    darknet_yolov5l,
    darknet_yolov5m,
    darknet_yolov5n,
    darknet_yolov5s,
    darknet_yolov5x,
)
from .vovnet import (
    ESEBlock,
    OSABlock,
    VoVNet,
    vovnet19_ese,
    vovnet19_slim_ese,
    vovnet27_slim,
    vovnet39,
    vovnet39_ese,
    vovnet57,
    vovnet57_ese,
    vovnet99_ese,
)
