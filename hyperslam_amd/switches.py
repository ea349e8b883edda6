"""The measurement switches of HS_DEBUG_FLAGS by name. The table is csrc/switches.hpp (one HS_SWITCH(name, bit, "meaning") line per
switch), read here as text: there is no second list.

    os.environ["HS_DEBUG_FLAGS"] = switches.flags("one_ended", "backward_sb")      # "4294969344"
    switches.names(4294969344)                                                      # ["one_ended", "backward_sb"]
"""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "switches.hpp")
_LINE = re.compile(r'^\s*HS_SWITCH\(\s*(\w+)\s*,\s*(\d+)\s*,\s*"([^"]*)"\s*\)', re.M)

with open(HEADER) as _f:
    TABLE = [(name, int(bit), meaning) for name, bit, meaning in _LINE.findall(_f.read())]  # in the header's order
VALUES = {name: 1 << bit for name, bit, _ in TABLE}    # name -> its value in HS_DEBUG_FLAGS
MEANINGS = {name: meaning for name, _, meaning in TABLE}


def value(*names):
    """The number that sets the named switches (none: 0). An unknown name is a KeyError."""
    v = 0
    for n in names:
        v |= VALUES[n]
    return v


def flags(*names):
    """The string for the environment variable HS_DEBUG_FLAGS: one decimal number."""
    return str(value(*names))


def names(number):
    """The names of the switches set in a number (or in a string of HS_DEBUG_FLAGS), in the table's order; a bit with two names gives both."""
    number = int(number)
    return [n for n, _, _ in TABLE if number & VALUES[n]]


def add_to_env(*names):
    """Sets the named switches in this process's HS_DEBUG_FLAGS, next to whatever it already holds; returns the new number."""
    number = value(*names) | int(os.environ.get("HS_DEBUG_FLAGS", "0"))
    os.environ["HS_DEBUG_FLAGS"] = str(number)
    return number
