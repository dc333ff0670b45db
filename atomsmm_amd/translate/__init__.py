"""Force translation: one OpenMM force object becomes backend objects, once, when the Context is created.

    table.py      the one table of force classes and the loops over it: translate, check_system, refuse_derivative, free_space_mode
    common.py     _Entry, pair_create / share_lists / make_bonded, globals_update, entry_of, the long-range corrections
    pair.py       NonbondedForce and the CustomNonbondedForce families, the pair-expression kernel
    terms.py      bonds, angles, torsions, external terms, compound bonds, CMAP, RB, RMSD
    allpairs.py   GBSAOBC, CustomGB, CustomHbond, CustomManyParticle, GayBerne, Drude

Every function here that needs the Context takes the engine as its first argument and uses these attributes of it, and no others:

    ctx, parameters, n, world, free_space, skin          the backend context and what the Context was created with
    box, _box_ref, _vscale                               for the long-range corrections (1 / V constants)
    _pair_info, shared                                   which pair forces may walk whose neighbour list
    entries, system, barostat                            what translation fills in
    _stock                                               check_system only: the stock integrator, if one steps the Context

Nothing here touches the engine's programs, memos, buffers or device scalars.  A closure left on an entry (update, reload, rescale)
says what it did by its result -- 'values', or True when bond-list terms were rebuilt -- and the engine reacts (Engine.set_parameter,
Engine.update_force_parameters)."""
from .allpairs import (GAYBERNE_MAX, GB_MAX_ATOMS, HBOND_MAX, MANY_MAX, MANY_MAX_NOCUTOFF, MANY_MAX_TYPES, MANY_PERMUTATIONS,  # noqa: F401
                       check_custom_gb_symmetry, drude_step_of, drude_tables, gayberne_tables, many_particle_table)
from .common import (_Entry, custom_long_range_correction, dispersion_correction, entry_of, globals_update, lrc_class_pairs,  # noqa: F401
                     make_bonded, share_lists, softcore_long_range_correction)
from .pair import check_pair_symmetry  # noqa: F401
from .table import CV_INNER_CLASSES, FORCE_TABLE, check_system, free_space_mode, refuse_derivative, translate, translate_cv  # noqa: F401
from .terms import RB_TEXT  # noqa: F401
