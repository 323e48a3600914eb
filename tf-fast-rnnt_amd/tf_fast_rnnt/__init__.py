"""tf_fast_rnnt on AMD MI355X (gfx950): the pruned RNN-T loss of Samsung/tf-fast-rnnt with its hot path
rebuilt as hand-written HIP behind a C ABI (include/ftr.h).  The public names, signatures and
``__version__`` are those of the reference package (tf_fast_rnnt/python/tf_fast_rnnt/__init__.py:24-36,
42,151); tensors are torch tensors on a HIP device (TensorFlow is not needed; a TF-ROCm op shim over the
same C ABI is described in INTEGRATION.md)."""
from ._lib import FtrError, lib as _load_native          # noqa: F401
from .mutual_information import cummin, mutual_information_recursion, mutual_information_viterbi   # the viterbi alignment: MI355X addition
from .mutual_information import mutual_information_recursion_multiblank   # MI355X addition: multi-blank (big blank) lattice
from .rnnt_loss import do_rnnt_pruning
from .rnnt_loss import do_rnnt_pruning_sum                                     # MI355X addition: am + lm[ranges] fused, f32 / bf16 / fp16
from .rnnt_loss import do_rnnt_pruning_act                                     # MI355X addition: tanh / relu of that sum, fused
from .rnnt_loss import get_rnnt_logprobs
from .rnnt_loss import get_rnnt_logprobs_joint
from .rnnt_loss import get_rnnt_logprobs_pruned
from .rnnt_loss import get_rnnt_logprobs_smoothed
from .rnnt_loss import get_rnnt_prune_ranges
from .rnnt_loss import get_hat_logprobs_joint, get_hat_logprobs_pruned, hat_loss, hat_loss_pruned  # MI355X addition: HAT loss, see hat_loss_pruned
from .rnnt_loss import get_rnnt_logprobs_multiblank_joint, get_rnnt_logprobs_multiblank_pruned   # MI355X addition: multi-blank
from .rnnt_loss import rnnt_loss_multiblank, rnnt_loss_multiblank_pruned                           # transducer loss, see there
from .mutual_information import mutual_information_recursion_tdt           # MI355X addition: token-and-duration (TDT) lattice
from .mutual_information import mutual_information_recursion_tdt_band      # ... and the same recursion on the pruned band itself
from .mutual_information import mutual_information_recursion_multiblank_band   # the multi-blank recursion on the pruned band
from .rnnt_loss import get_rnnt_logprobs_tdt_joint, get_rnnt_logprobs_tdt_pruned   # MI355X addition: TDT loss, a separate
from .rnnt_loss import rnnt_loss_tdt, rnnt_loss_tdt_pruned                         # duration head, see there
from .rnnt_loss import rnnt_loss_tdt_mixed, rnnt_loss_tdt_mixed_pruned             # ... mixed with the ordinary loss (omega)
from .mutual_information import mutual_information_viterbi_tdt              # MI355X addition: best-path alignment over the
from .mutual_information import mutual_information_viterbi_tdt_band         # ... and the same alignment on the pruned band itself
from .rnnt_loss import rnnt_alignment_tdt_pruned, rnnt_alignment_multiblank_pruned   # TDT / multi-blank lattices, see there
from .rnnt_loss import rnnt_loss
from .rnnt_loss import rnnt_loss_pruned
from .rnnt_loss import rnnt_kd_loss_pruned                                     # MI355X addition: distillation on the pruned band, see its docstring
from .rnnt_loss import rnnt_kd_loss_pruned_factored                            # ... for HAT and TDT rows, with node weights
from .rnnt_loss import rnnt_loss_pruned_kd                                     # ... and rnnt_loss_pruned + that loss in one pass over the student
from .rnnt_loss import rnnt_loss_pruned_kd_factored, rnnt_node_occupancy_pruned   # ... the same for HAT rows, node and occupancy weights
from .rnnt_loss import rnnt_kd_loss_pruned_topk, rnnt_kd_topk_teacher         # ... and from a stored top-K teacher on the teacher's own band
from .rnnt_loss import rnnt_alignment_pruned                           # MI355X addition: best-path alignment, see its docstring
from .rnnt_loss import rnnt_loss_simple
from .rnnt_loss import rnnt_loss_smoothed
from .rnnt_loss import tune_normalizer_gemms, normalizer_gemm_choice, set_normalizer_gemm_choice                # MI355X addition: library-GEMM kernel selection, see its docstring

__version__ = '1.2'

# Fail loudly at import if the HIP extension has not been built (no CPU fallback exists).
_load_native()
