"""Inputs of the dictionary page tests (tests/test_dictpages_host.py, tests/test_dictpages_gpu.py): the same bytes for the CPU model's
grid and for the GPU's.

Test infrastructure only.
"""
import dict_cases


def edge_input(dic, n=8192):
    """n bytes of text that start with the dictionary's last 300 bytes and end with another 300 of its bytes (all of it where it is
    shorter): the first page opens with a match into the dictionary and the last one ends in one"""
    dic = bytes(dic)
    head = dic[-300:]
    at = len(dic) // 3
    tail = dic[at: at + 300]
    return head + dict_cases.text(77000 + len(dic), n - len(head) - len(tail)) + tail
