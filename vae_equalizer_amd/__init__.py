"""vae_equalizer_amd -- MI355X-native (gfx950) hot path of kit-cel/vae-equalizer.

Only what the path needs: ``csrc/`` (HIP kernels + C ABI -> ``libvaeq_hip.so``), the ctypes binding
(``_native``), the batched run engines (``engine``) and host-side mirrors of the reference's call surface
(``shared_funcs``, ``func_VAELE_DP_MQAM_shaping``, ``func_VAEflex_DP_MQAM_shaping``, ``func_VAELE_MQAM_shaping``,
``Eval_run_DP``, ``Eval_run_shaping_vaele``, ``func_CMA_MQAM_shaping``, ``Eval_run_shaping_cma``, ``func_VAENN_MQAM``).  The VAE-NN encoder
classes ``Net`` / ``Net_BN`` (torch modules on the HIP kernels vaeq_nn_enc_forward / vaeq_nn_enc_backward), the functional ``nn_encode`` and the
converters ``net_to_theta`` / ``theta_to_net`` are re-exported here.  There is no CPU fallback: without the HIP library every
compute entry point raises.
"""
from . import _native  # noqa: F401
from .autograd_ops import nn_encode
from .func_VAENN_MQAM import Net, Net_BN, net_to_theta, theta_to_net

__all__ = ["_native", "Net", "Net_BN", "nn_encode", "net_to_theta", "theta_to_net"]
