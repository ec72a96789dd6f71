"""Copies derived from weights (operand-order packings, transposes, merged matrices, filled descriptors, captured graphs):
ONE rule for when a copy is current, ONE place where it is kept.  Host Python only.

The tag of an entry is, per source tensor t, id(t), t._version, t.data_ptr(), t.device, followed by the getter's `extra`
values.  It changes with an in-place write that autograd sees (an optimizer step), with a replaced Parameter object
(load_state_dict(assign=True), `module.weight = nn.Parameter(..)`) and with moved storage (.to(), .cuda(), _apply).  It does
NOT change with a write through `t.data` or a raw pointer (dist.broadcast(p.data, ..), EMA swaps, manual loaders): after one of
those, sparse.clear_packed_weights(module) — clear() below — is the contract.

Entries live on their owner (a tensor or a module) in one private attribute, {slot: (tag, value)}; every getter names its slot
with a string of its own.  The getters that run once per convolution launch read `module._parameters["weight"]`:
nn.Module.__getattr__ costs as much as the rest of a hit.
"""
_STORE = "_eprecon_derived"


def _tag(sources, extra):
    return [field for t in sources for field in (id(t), t._version, t.data_ptr(), t.device)] + list(extra)


def derived(owner, slot, sources, build, extra=()):
    """what build() made from the tensors `sources`, kept on `owner` under `slot` until the tag changes"""
    tag = []        # (_tag, written out: the hit path runs once per convolution launch and stays one frame deep)
    for t in sources:
        tag += (id(t), t._version, t.data_ptr(), t.device)
    tag += extra
    try:
        hit = owner.__dict__[_STORE][slot]
        if hit[0] == tag:
            return hit[1]
    except KeyError:
        pass
    value = build()
    owner.__dict__.setdefault(_STORE, {})[slot] = (tag, value)
    return value


def peek(owner, slot):
    """the value kept on `owner` under `slot`, current or not, or None; builds nothing"""
    return owner.__dict__.get(_STORE, {}).get(slot, (None, None))[1]


def current(owner, slot, sources, extra=()):
    """whether derived() with these arguments would be a hit"""
    return owner.__dict__.get(_STORE, {}).get(slot, (None, None))[0] == _tag(sources, extra)


def retag(owner, slot, sources, extra=()):
    """the value under `slot` has just been rewritten in place from `sources`: the entry counts as current"""
    store = owner.__dict__[_STORE]
    store[slot] = (_tag(sources, extra), store[slot][1])


def parameter_sources(module):
    """the live parameter tensors of a module tree.  Walking the tree costs ~0.25 ms per 100 modules, so WHERE they live is
    kept — each submodule's _parameters dict + name — in the module's own store: a Parameter object replaced later is seen,
    and clear() drops the list"""
    store = module.__dict__.setdefault(_STORE, {})
    if "weight_cache.parameter_slots" not in store:
        store["weight_cache.parameter_slots"] = (None, [(m._parameters, n) for m in module.modules() for n in m._parameters
                                                        if m._parameters[n] is not None])
    return [d[n] for d, n in store["weight_cache.parameter_slots"][1]]


def clear(module):
    """drop every entry kept on `module`, its submodules and their parameters"""
    for owner in (*module.modules(), *module.parameters()):
        owner.__dict__.pop(_STORE, None)
