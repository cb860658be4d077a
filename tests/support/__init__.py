"""Helpers that more than one test module (or a script under profiles/) uses.  Test modules import from here, never from each other."""
import pytest

# (the helpers carry most of the suite's assertions: keep pytest's operand introspection for them)
pytest.register_assert_rewrite("support.batches", "support.codeobj", "support.devmath", "support.gpu", "support.screen",
                               "support.sensors")
