"""Twin results of the lit / roulette image on the small scene of tests/plb_render_cases.py, computed once per process and shared by
tests/test_plb_render_light_cpu.py and tests/test_plb_render_light_gpu.py (never modified by a test)."""
import functools

import plb_render_cases as cases
from plb_render_light_twin import LightTwin

DEFAULT_LIGHT = (2.0, 1.0, 0.7)            # default_config.py:54


@functools.lru_cache(maxsize=None)
def light_twin(light=True, roulette=False, direction=DEFAULT_LIGHT, depth=2):
    return LightTwin(cases.render_conf(max_ray_depth=depth), light, roulette, direction)


@functools.lru_cache(maxsize=None)
def twin_image(light=True, roulette=False, seed=0, direction=DEFAULT_LIGHT, depth=2, nudge=0, spp=cases.SPP):
    tw = light_twin(light, roulette, direction, depth)
    return [tw.image(e, cases.twin_prims(b), spp=spp, seed=seed, nudge=nudge) for b, e in enumerate(cases.twin_bake())]
