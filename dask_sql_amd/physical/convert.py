"""RelConverter — plan-node → physical dispatch.

Mirrors the reference's physical/rel/convert.py:39-63 (dispatch keyed on
`rel.get_current_node_type()`) and utils.py Pluggable:61-91 plugin registry:
`add_plugin_class(cls, replace=True)` swaps in a converter for a node type —
the drop-in boundary of SURVEY.md §8b.
"""
from __future__ import annotations

import logging

logger = logging.getLogger(__name__)


class RelConverter:
    _plugins: dict = {}

    @classmethod
    def add_plugin_class(cls, plugin_class, replace=True):
        names = plugin_class.class_name
        if isinstance(names, str):
            names = [names]
        for name in names:
            if name in cls._plugins and not replace:
                continue
            cls._plugins[name] = plugin_class()

    @classmethod
    def convert(cls, rel, context):
        node_type = rel.get_current_node_type()
        try:
            plugin_instance = cls._plugins[node_type]
        except KeyError:
            raise NotImplementedError(
                f"No conversion for class {node_type} available (yet)"
            )
        logger.debug(
            f"Processing REL {node_type} using {plugin_instance.__class__.__name__}"
        )
        # Within one query, structurally equal Aggregate subtrees (a CTE or
        # view referenced twice) run once and share their result: float
        # SUMs accumulate in no fixed order, so a second run could differ
        # in the last bits and break `x = (SELECT MAX(x) FROM cte)`.
        memo = getattr(context, "_agg_memo", None)
        if memo is None or node_type != "Aggregate":
            return plugin_instance.convert(rel, context=context)
        key = rel.signature()
        if key not in memo:
            memo[key] = plugin_instance.convert(rel, context=context)
        return memo[key]


def _host_to_device(dc, context):
    """Re-upload a HostDataContainer (row order kept) as a DataContainer."""
    from dask_sql_amd.datacontainer import (ColumnContainer, DataContainer,
                                            HostDataContainer)
    if not isinstance(dc, HostDataContainer):
        return dc
    from dask_sql_amd.context import RegisteredTable, _from_pandas
    names = [str(c) for c in dc.pdf.columns]
    backend = [f"h{i}__{n}" for i, n in enumerate(names)]
    pdf = dc.pdf.set_axis(backend, axis=1).reset_index(drop=True)
    table = RegisteredTable(_from_pandas(pdf)).upload(context._get_runtime())
    return DataContainer(table, ColumnContainer(names,
                                                dict(zip(names, backend))))


class BaseRelPlugin:
    """reference physical/rel/base.py:25-124 contract."""

    class_name: str | list = None

    def convert(self, rel, context):
        raise NotImplementedError

    @staticmethod
    def assert_inputs(rel, n=1, context=None, host_ok=False):
        # reference rel/base.py:67-86: depth-first recursion over inputs.
        # A Sort/Limit below (derived table, hidden ORDER BY column) hands
        # back a host frame; only plugins that say host_ok take it as is,
        # every other one gets it back as device columns.
        input_rels = rel.get_inputs()
        assert len(input_rels) == n, (len(input_rels), n)
        dcs = [RelConverter.convert(r, context) for r in input_rels]
        if not host_ok:
            dcs = [_host_to_device(dc, context) for dc in dcs]
        return dcs

    @staticmethod
    def fix_column_to_row_type(cc, row_type):
        # reference rel/base.py:32-51: rename to the rel's field names
        field_names = [str(f) for f in row_type.getFieldNames()]
        cc = cc.rename(dict(zip(cc.columns, field_names)))
        return cc.limit_to(field_names)
