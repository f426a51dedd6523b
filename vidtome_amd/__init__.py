"""vidtome_amd -- MI355X-native implementation of VidToMe's cross-frame token-merging hot path.

Same public surface as the reference's ``vidtome`` package (vidtome/__init__.py:1-4):
``apply_patch, remove_patch, update_patch, collect_from_patch`` plus the ``merge`` and ``patch`` modules.
Everything executes in libvidtome_hip.so (hand-written HIP for gfx950); there is no CPU fallback.
"""
from . import merge, patch
from .patch import apply_patch, remove_patch, update_patch, collect_from_patch
from .maps import register_attention_maps, unregister_attention_maps
from .p2p import CrossEdit, register_cross_attention_control, unregister_cross_attention_control
from .blend import LocalBlend, register_local_blend, unregister_local_blend
from .sampler import GuidedDDIM, GuidedDPMSolver
from .inversion import EditFriendlyInversion
from .noise import FrameNoise
from .pag import register_perturbed_attention, remove_perturbed_attention
from .sag import SelfAttentionGuidance, register_self_attention_guidance, unregister_self_attention_guidance
from .freeu import register_freeu, unregister_freeu
from .semantic import EditConcept, SemanticGuidance
from .broadcast import AttentionBroadcast, register_attention_broadcast, unregister_attention_broadcast

__all__ = ["merge", "patch", "apply_patch", "remove_patch", "update_patch", "collect_from_patch",
           "register_attention_maps", "unregister_attention_maps",
           "CrossEdit", "register_cross_attention_control", "unregister_cross_attention_control",
           "LocalBlend", "register_local_blend", "unregister_local_blend",
           "GuidedDDIM", "GuidedDPMSolver", "register_perturbed_attention", "remove_perturbed_attention",
           "SelfAttentionGuidance", "register_self_attention_guidance", "unregister_self_attention_guidance",
           "register_freeu", "unregister_freeu", "EditConcept", "SemanticGuidance", "EditFriendlyInversion", "FrameNoise",
           "AttentionBroadcast", "register_attention_broadcast", "unregister_attention_broadcast"]
