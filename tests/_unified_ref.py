"""Checker-only restatement of the KG carriers' data path (paths relative to the reference's
HD_SELFRec tree), in NumPy / scipy without pandas:

* :func:`knowledge` — ``Knowledge.construct_data`` (data/knowledge.py:44-129): the five-block
  triple table in the reference's order, its counts, the h / t / r lists, ``train_kg_dict``,
  and the first-appearance maps of entities and relations;
* :func:`kg_interaction_mat` / :func:`normalize_graph_mat` — knowledge.py:135-148 and
  data/graph.py:11-25 with scipy, as the reference calls it;
* :func:`next_batch_unified` — util/sampler.py:7-90, driven by the real ``random`` and
  ``np.random`` so that the 2-D shuffle's degenerate row swap and the set orders come out of
  CPython and NumPy themselves. It yields lists of Python ints instead of tensors.

An empty KG has no ``max(r)``: the reference raises there; this restatement (and the library)
takes ``n_relations`` of the raw KG as 0, so the table is the two CF blocks alone.
"""
import collections
import random
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp


def knowledge(training, h, r, t):
    h = np.asarray(h, dtype=np.int64)
    r = np.asarray(r, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    cf = np.array([[rec[0], rec[1]] for rec in training], dtype=np.int64).reshape(-1, 2)
    n0 = int(r.max()) + 1 if r.size else 0
    kg = np.stack([h, r, t], axis=1)                      # kg_data
    inv = np.stack([t, r + n0, h], axis=1)                # inverse_kg_data, r += n_relations
    both = np.concatenate([kg, inv])                      # first concat
    both[:, 1] += 2                                       # kg_data['r'] += 2
    kg_train = np.concatenate([both, inv])                # second concat: inverse WITHOUT the +2
    n_entities = int(max(kg_train[:, 0].max(), kg_train[:, 2].max())) + 1 if len(kg_train) else 0
    cf2kg = np.stack([cf[:, 0], np.zeros(len(cf), np.int64), cf[:, 1]], axis=1)
    inv_cf2kg = np.stack([cf[:, 1], np.ones(len(cf), np.int64), cf[:, 0]], axis=1)
    data = np.concatenate([kg_train, cf2kg, inv_cf2kg])
    k = SimpleNamespace(kg_train_data=data, n_kg_train=len(data), n_entities=n_entities)
    k.n_users_entities = int(max(data[:, 0].max(), data[:, 2].max())) + 1 if len(data) else 0
    k.n_relations = int(data[:, 1].max()) + 1 if len(data) else 0
    k.entity, k.relation = {}, {}
    k.train_kg_dict = collections.defaultdict(list)
    k.h_list, k.t_list, k.r_list = [], [], []
    for row in data.tolist():                             # the iterrows loop
        hh, rr, tt = row
        k.h_list.append(hh)
        k.t_list.append(tt)
        k.r_list.append(rr)
        if hh not in k.entity:
            k.entity[hh] = len(k.entity)
        if tt not in k.entity:
            k.entity[tt] = len(k.entity)
        if rr not in k.relation:
            k.relation[rr] = len(k.relation)
        k.train_kg_dict[hh].append((tt, rr))
    return k


def kg_interaction_mat(k):
    n = max(k.n_users_entities, 1)
    return sp.csr_matrix((np.ones(len(k.h_list)), (k.h_list, k.t_list)), shape=(n, n),
                         dtype=np.float32)


def normalize_graph_mat(adj_mat):
    shape = adj_mat.get_shape()
    rowsum = np.array(adj_mat.sum(1))
    with np.errstate(divide="ignore"):
        if shape[0] == shape[1]:
            d_inv = np.power(rowsum, -0.5).flatten()
            d_inv[np.isinf(d_inv)] = 0.
            d_mat_inv = sp.diags(d_inv)
            norm_adj_tmp = d_mat_inv.dot(adj_mat)
            return norm_adj_tmp.dot(d_mat_inv)
        d_inv = np.power(rowsum, -1).flatten()
        d_inv[np.isinf(d_inv)] = 0.
        return sp.diags(d_inv).dot(adj_mat)


def next_batch_unified(data, data_kg, batch_size, batch_size_kg, n_negs=1):
    ptr = 0
    cf_data = np.array(data.training_data)
    kg_data = np.array(data_kg.kg_train_data)             # DataFrame.to_numpy(): a 2-D array
    cf_size = len(cf_data)

    random.shuffle(kg_data)
    random.shuffle(cf_data)

    lst_user_item = list(set(list(cf_data[:, 0]) + list(cf_data[:, 1])))
    train_kg_dict = {k: data_kg.train_kg_dict[k] for k in lst_user_item}
    h_list = list(train_kg_dict.keys())
    h_dict = {value: idx for idx, value in enumerate(h_list)}

    all_tails = []
    pos_tail_sets = {}
    for head, tails in train_kg_dict.items():
        all_tails += [it[0] for it in tails]
        pos_tail_sets[head] = set([it[0] for it in tails])
    all_tails = list(set(all_tails))

    while ptr < cf_size:
        batch_end = ptr + batch_size if ptr + batch_size < cf_size else cf_size
        users = cf_data[ptr:batch_end, 0]
        items = cf_data[ptr:batch_end, 1]
        ptr = batch_end

        u_idx, i_idx, j_idx = [], [], []
        item_list = list(data.item.keys())
        for i, user in enumerate(users):
            i_idx.append(data.item[items[i]])
            u_idx.append(data.user[user])
            for _ in range(n_negs):
                neg_item = random.choice(item_list)
                while neg_item in data.training_set_u[user]:
                    neg_item = random.choice(item_list)
                j_idx.append(data.item[neg_item])

        selected_kg_data = []
        for h in train_kg_dict.keys():
            for val in train_kg_dict[h]:
                selected_kg_data.append([int(h), val[1], val[0]])
        selected_kg_data = np.array(selected_kg_data)
        selected_indices = np.random.randint(len(selected_kg_data), size=batch_size_kg)
        selected_kg_data = selected_kg_data[selected_indices, :]
        heads, relations, tails = (selected_kg_data[:, 0], selected_kg_data[:, 1],
                                   selected_kg_data[:, 2])
        h_idx = [h_dict[int(h)] for h in heads]
        r_idx = [int(rel) for rel in relations]
        pos_t_idx = [int(tail) for tail in tails]
        neg_t_idx = []
        for head in heads:
            neg_t = random.choice(all_tails)
            while neg_t in pos_tail_sets[head]:
                neg_t = random.choice(all_tails)
            neg_t_idx.append(int(neg_t))
        yield u_idx, i_idx, j_idx, h_idx, r_idx, pos_t_idx, neg_t_idx, h_list
