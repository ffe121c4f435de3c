"""The numpy twin's result on every case of smooth_inputs.py (computed once, shared, never modified)."""
import smooth_inputs as sm

_twins = {}


def twin(name):
    """ClusterResult of euclidean_clusters_host on the case with scores_of(name)."""
    from randlanet.utils.cluster import euclidean_clusters_host
    if name not in _twins:
        xyz, labels, r, kw = sm.case(name)
        _twins[name] = euclidean_clusters_host(xyz, labels, radius=r, scores=sm.scores_of(name), **kw)
    return _twins[name]
