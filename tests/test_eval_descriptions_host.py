"""Host side of the ten vaek_*_replicas evaluation entry points, no GPU: each checks its description before its context, in one order."""
import pytest

from tests.abi_util import check_description_guard

ENTRIES = ("vaek_stats_event_replicas", "vaek_mlp3_stats_event_replicas", "vaek_log_likelihood_replicas", "vaek_mlp3_log_likelihood_replicas",
           "vaek_spectrum_event_replicas", "vaek_eigen_event_replicas", "vaek_exact_log_likelihood_replicas", "vaek_elbo_hvp_replicas",
           "vaek_elbo_hessian_lanczos_replicas", "vaek_mlp3_decoder_jacobian_replicas")


@pytest.mark.parametrize("name", ENTRIES)
def test_the_description_is_checked_before_the_context(name):
    """With a NULL context: a NULL description gives -1 and the entry's name; a struct_size eight bytes short gives -1, the name and
    `struct_size <got> != <want>` with <want> the ctypes mirror's size; the right size gives -1 and "null context"."""
    from vae_training_amd import _lib
    check_description_guard(_lib.load(), name)
