"""CPU: the model registry lists the models and nothing else -- a module of models/ that holds shared code (wsgan_shared.py) is no model,
neither in the list nor in the refusal that quotes it -- and every listed wsgan baseline resolves to its class by name."""
import pytest


def test_available_models_and_their_classes():
    from pcgan_amd import models
    from pcgan_amd.util.registry import available
    assert available('pcgan_amd.models', 'model') == ['wsgan_bigan', 'wsgan_cont', 'wsgan_cycle', 'wsgan_disc', 'wsgan_emb']
    with pytest.raises(NotImplementedError, match=r'\(available: wsgan_bigan, wsgan_cont, wsgan_cycle, wsgan_disc, wsgan_emb\)'):
        models.find_model_using_name('wsgan_shared')
    for name, cls in (('wsgan_bigan', 'WSGANBiGANModel'), ('wsgan_cont', 'WSGANContModel'), ('wsgan_cycle', 'WSGANCycleModel'),
                      ('wsgan_disc', 'WSGANDiscModel')):
        found = models.find_model_using_name(name)
        assert found.__name__ == cls and found.__module__ == 'pcgan_amd.models.%s_model' % name and found().name() == cls
        assert callable(models.get_option_setter(name))
